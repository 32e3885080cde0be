// tree_check.cpp — the tree-quality ABI's arithmetic (pt_tree_math.hpp, the
// functions the kernels of pt_tree.hip call) run on the CPU in the kernels'
// order: a stand-alone host program, no HIP, no GPU. `make tree_check` builds
// it; tests/test_tree_abi.py compares its output with the numpy reference bit
// for bit.
//
//   tree_check areas  ref_nodes.f32 out.f32
//   tree_check growth ref_nodes.f32 base.f32 out.f32
//   tree_check remap  ids.i32 map_spheres.i32 map_tris.i32 map_quads.i32 out.i32
//
// Files are raw little-endian 4-byte words (f32, or i32 where named so);
// ref_nodes is a whole number of 12-word rows, base one f32 per row; a map's
// count is its file's length. growth runs the 1024 lanes of tree_growth one
// after the other and then the reduction for s = 512 .. 1. Exit 0 on success,
// 2 on bad arguments or I/O.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ptmi_tree.h"
#include "pt_check_io.hpp"
#include "pt_tree_math.hpp"

using namespace ptmi;

// The words of a file as they are: an i32 file read as f32 keeps its bits (no arithmetic touches them).
static bool read_words(const char* path, std::vector<float>& v) { return read_all_f32(path, v); }

static std::vector<int32_t> as_i32(const std::vector<float>& v) {
  std::vector<int32_t> w(v.size());
  if (!v.empty()) memcpy(w.data(), v.data(), 4 * v.size());
  return w;
}

static int usage(const char* prog) {
  fprintf(stderr,
          "usage: %s areas ref_nodes.f32 out.f32 | growth ref_nodes.f32 base.f32 out.f32 | "
          "remap ids.i32 map_spheres.i32 map_tris.i32 map_quads.i32 out.i32\n",
          prog);
  return 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage(argv[0]);
  const char* mode = argv[1];
  std::vector<float> out;
  const char* dst = nullptr;
  if (!strcmp(mode, "areas") || !strcmp(mode, "growth")) {
    const bool growth = mode[0] == 'g';
    if (argc != (growth ? 5 : 4)) return usage(argv[0]);
    std::vector<float> ref, base;
    if (!read_words(argv[2], ref) || ref.size() % kTreeRefFloats) {
      fprintf(stderr, "cannot read whole rows of %d f32\n", kTreeRefFloats);
      return 2;
    }
    const int32_t n = (int32_t)(ref.size() / kTreeRefFloats);
    if (!growth) {
      dst = argv[3];
      for (int32_t i = 0; i < n; ++i) out.push_back(tree_area(ref.data() + (size_t)i * kTreeRefFloats));
    } else {
      dst = argv[4];
      if (!read_words(argv[3], base) || base.size() != (size_t)n) {
        fprintf(stderr, "base must hold one f32 per row\n");
        return 2;
      }
      const int lanes = PTMI_TREE_GROWTH_LANES;
      std::vector<TreeAcc> acc(lanes);
      for (int k = 0; k < lanes; ++k) acc[k] = tree_lane(ref.data(), base.data(), n, k, lanes);
      for (int s = lanes / 2; s >= 1; s >>= 1)
        for (int k = 0; k < s; ++k) tree_combine(acc[k], acc[k + s]);
      out.resize(4);
      tree_finish(acc[0], out.data());
    }
  } else if (!strcmp(mode, "remap")) {
    if (argc != 7) return usage(argv[0]);
    std::vector<float> w[4];
    for (int j = 0; j < 4; ++j)
      if (!read_words(argv[2 + j], w[j])) {
        fprintf(stderr, "cannot read %s\n", argv[2 + j]);
        return 2;
      }
    const std::vector<int32_t> ids = as_i32(w[0]), ms = as_i32(w[1]), mt = as_i32(w[2]), mq = as_i32(w[3]);
    const TreeMaps maps = {ms.data(), mt.data(), mq.data(), (int32_t)ms.size(), (int32_t)mt.size(), (int32_t)mq.size()};
    std::vector<int32_t> got(ids.size());
    for (size_t i = 0; i < ids.size(); ++i) got[i] = tree_remap_id(ids[i], maps);
    out.resize(got.size());
    if (!got.empty()) memcpy(out.data(), got.data(), 4 * got.size());
    dst = argv[6];
  } else {
    fprintf(stderr, "unknown mode %s\n", mode);
    return 2;
  }
  if (!write_f32(dst, out)) {
    fprintf(stderr, "cannot write the output\n");
    return 2;
  }
  return 0;
}
