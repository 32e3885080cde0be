// pt_tree_math.hpp — the arithmetic of the tree-quality ABI
// (include/ptmi_tree.h): the area of a ref_nodes row's box, an internal node's
// growth against its baseline, the walk of one lane of ptmi_tree_growth and the
// step of its reduction, and the remap of one id. Stated once here for the
// kernels of pt_tree.hip and for the CPU program tree_check.cpp.
//
// Compiled with -ffp-contract=off and a correctly rounded f32 division: one
// rounding per operation, as in the numpy reference (tests/tree_helpers.py).
#ifndef PT_TREE_MATH_HPP
#define PT_TREE_MATH_HPP

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PTMI_TREE_HD __host__ __device__ __forceinline__
#else
#define PTMI_TREE_HD inline
#endif

namespace ptmi {

constexpr int kTreeRefFloats = 12;  // a ref_nodes row (include/ptmi.h)

PTMI_TREE_HD int32_t tree_word(float f) {
  int32_t w;
  memcpy(&w, &f, 4);
  return w;
}

// A(i) of the header: row = {min.xyz, left | max.xyz, right | ...}.
PTMI_TREE_HD float tree_area(const float* row) {
  const float dx = row[4] - row[0], dy = row[5] - row[1], dz = row[6] - row[2];
  return 2.0f * ((dx * dy + dy * dz) + dz * dx);
}

PTMI_TREE_HD bool tree_is_inner(const float* row) { return tree_word(row[3]) >= 0; }

// r(i): the row's area now over its baseline area, 1 where there is no baseline.
PTMI_TREE_HD float tree_term(const float* row, float base) { return base > 0.0f ? tree_area(row) / base : 1.0f; }

PTMI_TREE_HD float tree_max(float a, float b) { return (a > b) ? a : b; }

// What one lane, and after the reduction the workgroup, holds.
struct TreeAcc {
  double sum;
  float mx;
  int32_t n;
};

// Step 1: lane k of `lanes` walks rows k, k + lanes, ... below n_nodes.
PTMI_TREE_HD TreeAcc tree_lane(const float* ref_nodes, const float* base, int32_t n_nodes, int32_t k, int32_t lanes) {
  TreeAcc a = {0.0, 1.0f, 0};
  for (int64_t i = k; i < n_nodes; i += lanes) {
    const float* row = ref_nodes + (size_t)i * kTreeRefFloats;
    if (!tree_is_inner(row)) continue;
    const float r = tree_term(row, base[i]);
    a.sum += (double)r;
    a.mx = tree_max(a.mx, r);
    a.n += 1;
  }
  return a;
}

// Step 2: what lane k does with lane k + s's values.
PTMI_TREE_HD void tree_combine(TreeAcc& a, const TreeAcc& b) {
  a.sum += b.sum;
  a.mx = tree_max(a.mx, b.mx);
  a.n += b.n;
}

// Step 3: out[4] of the reduced values.
PTMI_TREE_HD void tree_finish(const TreeAcc& a, float* out) {
  out[0] = a.n > 0 ? (float)(a.sum / (double)a.n) : 1.0f;
  out[1] = a.mx;
  out[2] = (float)a.n;
  out[3] = 0.0f;
}

// The three maps and counts of ptmi_ids_remap, by name so that a lane selects
// rather than indexes them.
struct TreeMaps {
  const int32_t *spheres, *tris, *quads;  // type 0, 1, 2
  int32_t num_spheres, num_tris, num_quads;
};

// One id through its type's map. The map is read only for a prim inside its count.
PTMI_TREE_HD int32_t tree_remap_id(int32_t id, const TreeMaps& t) {
  if (id < 0) return -1;
  const int32_t type = id >> 28, prim = id & 0x0fffffff;
  if (type > 2) return -1;
  const int32_t count = type == 0 ? t.num_spheres : type == 1 ? t.num_tris : t.num_quads;
  if (prim >= count) return -1;
  const int32_t* map = type == 0 ? t.spheres : type == 1 ? t.tris : t.quads;
  const int32_t m = map[prim];
  if (m < 0 || m >= count) return -1;
  return (int32_t)((uint32_t)type << 28) | m;
}

}  // namespace ptmi
#endif  // PT_TREE_MATH_HPP
