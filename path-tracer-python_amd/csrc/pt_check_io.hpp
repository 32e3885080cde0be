// pt_check_io.hpp — the raw little-endian f32 files of the CPU check programs
// (denoise_check.cpp, reproject_check.cpp, update_check.cpp, motion_check.cpp,
// tree_check.cpp, validate_check.cpp, material_check.cpp).
// Host only.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

// Reads exactly v.size() values: false if the file is shorter or longer.
inline bool read_f32(const char* path, std::vector<float>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), sizeof(float), v.size(), f);
  const bool at_end = fgetc(f) == EOF;
  fclose(f);
  return got == v.size() && at_end;
}

// The same for raw little-endian i32 (motion_check.cpp's id images).
inline bool read_i32(const char* path, std::vector<int32_t>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), sizeof(int32_t), v.size(), f);
  const bool at_end = fgetc(f) == EOF;
  fclose(f);
  return got == v.size() && at_end;
}

// Appends a whole file to v: false if it is not a whole number of values.
inline bool read_all_f32(const char* path, std::vector<float>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  float buf[1024];
  size_t got;
  while ((got = fread(buf, sizeof(float), 1024, f)) > 0) v.insert(v.end(), buf, buf + got);
  const bool whole = feof(f) && ftell(f) % (long)sizeof(float) == 0;
  fclose(f);
  return whole;
}

inline bool write_f32(const char* path, const std::vector<float>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const size_t put = fwrite(v.data(), sizeof(float), v.size(), f);
  return fclose(f) == 0 && put == v.size();
}
