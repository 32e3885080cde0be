// pose_check.cpp — the pose ABI's arithmetic (pt_pose_math.hpp, the functions
// the kernel of pt_pose.hip calls) run on the CPU: a stand-alone host program,
// no HIP, no GPU. `make pose_check` builds it; tests/test_pose_check.py compares
// its output with the Python definition (ptmi/pose.py) bit for bit.
//
//   pose_check MODE T in.f64 out.f32
//
// T is the shutter time as strtod reads it (a hex float keeps every bit).
// in.f64 is raw little-endian f64, a whole number of records: the track record
// of include/ptmi_pose.h followed by the row floats the kernel reads, as f64:
//   sphere   7 {o, d, r}            -> 9 f32 {c.xyz, mn.xyz, mx.xyz}
//   quad    15 {Q, d, normal, u, v} -> 10 f32 {D, Q.xyz, mn.xyz, mx.xyz}
//   tri     12 {v0, v1, v2, d}      -> 9 f32 {v0.xyz, mn.xyz, mx.xyz}
// Exit 0 on success, 2 on bad arguments or I/O.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pt_check_io.hpp"
#include "pt_pose_math.hpp"

using namespace ptmi;

static bool read_all_f64(const char* path, std::vector<double>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  double buf[512];
  size_t got;
  while ((got = fread(buf, sizeof(double), 512, f)) > 0) v.insert(v.end(), buf, buf + got);
  const bool whole = feof(f) && ftell(f) % (long)sizeof(double) == 0;
  fclose(f);
  return whole;
}

static void put_box(std::vector<float>& out, const UpdBox& b) {
  out.insert(out.end(), b.mn, b.mn + 3);
  out.insert(out.end(), b.mx, b.mx + 3);
}

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s sphere|quad|tri T in.f64 out.f32\n", argv[0]);
    return 2;
  }
  const char* mode = argv[1];
  const size_t rec = !strcmp(mode, "sphere") ? 7 : !strcmp(mode, "quad") ? 15 : !strcmp(mode, "tri") ? 12 : 0;
  if (!rec) {
    fprintf(stderr, "unknown mode %s\n", mode);
    return 2;
  }
  char* end = nullptr;
  const double t = strtod(argv[2], &end);
  if (end == argv[2] || *end || !isfinite(t)) {
    fprintf(stderr, "T must be a finite number\n");
    return 2;
  }
  std::vector<double> in;
  std::vector<float> out;
  if (!read_all_f64(argv[3], in) || in.size() % rec) {
    fprintf(stderr, "cannot read whole records of %zu f64\n", rec);
    return 2;
  }
  for (size_t i = 0; i < in.size(); i += rec) {
    const double* r = in.data() + i;
    if (rec == 7) {
      float row[4] = {0.0f, 0.0f, 0.0f, (float)r[6]};
      const UpdBox b = pose_sphere(r, t, row);
      out.insert(out.end(), row, row + 3);
      put_box(out, b);
    } else if (rec == 15) {
      float row[16] = {0.0f};
      for (int k = 0; k < 6; ++k) row[7 + k] = (float)r[9 + k];
      const UpdBox b = pose_quad(r, t, row);
      out.insert(out.end(), row + 3, row + 7);
      put_box(out, b);
    } else {
      float row[12] = {0.0f};
      const UpdBox b = pose_tri(r, t, row);
      out.insert(out.end(), row, row + 3);
      put_box(out, b);
    }
  }
  if (!write_f32(argv[4], out)) {
    fprintf(stderr, "cannot write the output\n");
    return 2;
  }
  return 0;
}
