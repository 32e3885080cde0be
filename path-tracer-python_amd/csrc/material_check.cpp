// material_check.cpp — the material-edit ABI's integer rules
// (pt_material_math.hpp and, for the leaf code, pt_scene_rows.hpp: the
// functions the kernel of pt_material.hip calls) run on the CPU: a stand-alone
// host program, no HIP, no GPU. `make material_check` builds it;
// tests/test_material_abi.py compares its output with
// scene_data.material_class and scene_data.leaf_code.
//
//   material_check classes flags.u32 out.u32
//   material_check patch   codes.u32 classes.u32 out.u32
//   material_check names   codes.u32 types.i32 prims.i32 out.u32
//   material_check images  flags.u32 num_images out.u32
//
// Files are raw little-endian 4-byte words, one per case; the inputs of one
// mode have the same length. classes: mat_class of every flags word. patch:
// leaf_patch_class of every (code, class). names: 1 where leaf_code_names holds.
// images: 1 where mat_image_ok holds. Exit 0 on success, 2 on bad arguments or
// I/O.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pt_check_io.hpp"
#include "pt_material_math.hpp"

using namespace ptmi;

// The words of a file as they are: read as f32 they keep their bits (no arithmetic touches them).
static bool read_words(const char* path, std::vector<uint32_t>& w) {
  std::vector<float> v;
  if (!read_all_f32(path, v)) return false;
  w.resize(v.size());
  if (!v.empty()) memcpy(w.data(), v.data(), 4 * v.size());
  return true;
}

static bool write_words(const char* path, const std::vector<uint32_t>& w) {
  std::vector<float> v(w.size());
  if (!w.empty()) memcpy(v.data(), w.data(), 4 * w.size());
  return write_f32(path, v);
}

static int usage(const char* prog) {
  fprintf(stderr,
          "usage: %s classes flags.u32 out.u32 | patch codes.u32 classes.u32 out.u32 | "
          "names codes.u32 types.i32 prims.i32 out.u32 | images flags.u32 num_images out.u32\n",
          prog);
  return 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage(argv[0]);
  const char* mode = argv[1];
  const bool images = !strcmp(mode, "images");
  const int n_in = !strcmp(mode, "classes") ? 1 : !strcmp(mode, "patch") ? 2 : !strcmp(mode, "names") ? 3 : images ? 1 : 0;
  if (n_in == 0) {
    fprintf(stderr, "unknown mode %s\n", mode);
    return 2;
  }
  if (argc != 3 + n_in + (images ? 1 : 0)) return usage(argv[0]);
  std::vector<uint32_t> in[3];
  for (int j = 0; j < n_in; ++j)
    if (!read_words(argv[2 + j], in[j]) || in[j].size() != in[0].size()) {
      fprintf(stderr, "cannot read %s, or its length differs from the first input's\n", argv[2 + j]);
      return 2;
    }
  const int32_t num_images = images ? (int32_t)strtol(argv[3], nullptr, 10) : 0;
  std::vector<uint32_t> out(in[0].size());
  for (size_t i = 0; i < out.size(); ++i) {
    if (n_in == 2)
      out[i] = leaf_patch_class(in[0][i], in[1][i]);
    else if (n_in == 3)
      out[i] = leaf_code_names(in[0][i], (int32_t)in[1][i], (int32_t)in[2][i]) ? 1u : 0u;
    else
      out[i] = images ? (mat_image_ok(in[0][i], num_images) ? 1u : 0u) : mat_class(in[0][i]);
  }
  if (!write_words(argv[argc - 1], out)) {
    fprintf(stderr, "cannot write the output\n");
    return 2;
  }
  return 0;
}
