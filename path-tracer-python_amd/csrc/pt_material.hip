// pt_material.hip — the material-edit ABI (include/ptmi_material.h): mats rows
// of a resident scene replaced in place, and the leaf codes that carry each
// primitive's material class patched with them.
//
//   * mat_edit: one lane per edit of the three lists: the 20-f32 row is copied
//     over the primitive's mats row, the class of its new flags word replaces
//     the class bits of the leaf code in ref_nodes (the stackless traversal's
//     copy) and in the parent's nodes row (the stack traversal's). An edit
//     whose ids are out of range, whose leaf does not hold that primitive or
//     whose flags name an image the scene does not have is skipped.
//
// The integer rules are pt_material_math.hpp's, shared with material_check.cpp.
// A few thousand lanes of loads and vector stores: no LDS, no cross-lane reads,
// nothing timed by ptmi_prof_*. No render kernel is involved.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_material.h"
#include "pt_args.hpp"
#include "pt_material_math.hpp"

namespace ptmi {

constexpr int kMatBlock = 256;

// One list of edits as a kernel argument, with what its type fixes.
struct MatList {
  const int32_t* prim;
  const int32_t* leaf;
  const float* row;
  int32_t count;
  int32_t num_prims;
  int32_t type;  // the type code of a leaf: 0 sphere, 1 triangle, 2 quad
  int32_t base;  // the type's first row of mats (storage order: spheres, quads, triangles)
};

__global__ __launch_bounds__(kMatBlock) void mat_edit(MatList s, MatList q, MatList t, float* __restrict__ mats,
                                                      float* __restrict__ ref_nodes, float* __restrict__ nodes,
                                                      const int32_t* __restrict__ slot, int32_t num_bvh_nodes,
                                                      int32_t n_inner, int32_t num_images) {
  int32_t i = (int32_t)(blockIdx.x * (uint32_t)kMatBlock + threadIdx.x);
  MatList e = s;
  if (i >= s.count) {
    i -= s.count;
    e = q;
    if (i >= q.count) {
      i -= q.count;
      e = t;
      if (i >= t.count) return;
    }
  }
  const int32_t p = e.prim[i], leaf = e.leaf[i];
  if (p < 0 || p >= e.num_prims || leaf < 0 || leaf >= num_bvh_nodes) return;
  float* ref = ref_nodes + (size_t)leaf * kMatRefFloats;
  const uint32_t code = __float_as_uint(ref[9]);
  if (!mat_code_names(code, e.type, p)) return;
  const float* row = e.row + (size_t)i * kMatFloats;
  const uint32_t flags = __float_as_uint(row[kMatFloats - 1]);
  if (!mat_image_ok(flags, num_images)) return;
  float* dst = mats + ((size_t)e.base + (size_t)p) * kMatFloats;
  for (int k = 0; k < kMatFloats; ++k) dst[k] = row[k];
  const float patched = __uint_as_float(mat_patch_code(code, mat_class(flags)));
  const int32_t parent = __float_as_int(ref[8]), side = __float_as_int(ref[10]);
  ref[9] = patched;
  // the stack traversal's copy: child ref `side` of the parent's nodes row; the root has none
  if (n_inner <= 0 || parent < 0 || parent >= num_bvh_nodes || (side != 0 && side != 1)) return;
  const int32_t sl = slot[parent];
  if (sl < 0 || sl >= n_inner) return;
  nodes[(size_t)sl * kMatNodeFloats + 12 + side] = patched;
}

static bool mat_fill(MatList& d, const ptmi_material_list* s, int32_t num_prims, int32_t type, int64_t base) {
  d.prim = s ? s->prim : nullptr;
  d.leaf = s ? s->leaf : nullptr;
  d.row = s ? s->row : nullptr;
  d.count = s ? s->count : 0;
  d.num_prims = num_prims;
  d.type = type;
  d.base = (int32_t)base;
  return d.count >= 0 && d.count <= num_prims;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_update_materials(const ptmi_scene_view* scene, const ptmi_material_list* spheres,
                          const ptmi_material_list* quads, const ptmi_material_list* tris, const int32_t* slot,
                          void* stream) {
  if (!scene) return fail(PTMI_EINVAL, "materials: scene is NULL");
  if (scene->n_inner < 0 || scene->num_bvh_nodes < 0 || scene->num_spheres < 0 || scene->num_quads < 0 ||
      scene->num_triangles < 0 ||
      (int64_t)scene->num_spheres + scene->num_quads + scene->num_triangles > 0x7fffffff)
    return fail(PTMI_EINVAL, "materials: bad scene counts");
  MatList s, q, t;
  if (!mat_fill(s, spheres, scene->num_spheres, 0, 0))
    return fail(PTMI_EINVAL, "materials: sphere count negative or above num_spheres");
  if (!mat_fill(q, quads, scene->num_quads, 2, scene->num_spheres))
    return fail(PTMI_EINVAL, "materials: quad count negative or above num_quads");
  if (!mat_fill(t, tris, scene->num_triangles, 1, (int64_t)scene->num_spheres + scene->num_quads))
    return fail(PTMI_EINVAL, "materials: triangle count negative or above num_triangles");
  const struct {
    const MatList& l;
    const char* name;
  } lists[3] = {{s, "sphere"}, {q, "quad"}, {t, "triangle"}};
  for (const auto& e : lists)
    if (e.l.count > 0 && (bad4(e.l.prim) || bad4(e.l.leaf) || bad4(e.l.row)))
      return fail(PTMI_EINVAL, "materials: a %s list pointer is NULL/misaligned", e.name);
  const int64_t n_edits = (int64_t)s.count + q.count + t.count;
  if (n_edits == 0) return PTMI_OK;
  if (bad4(scene->mats)) return fail(PTMI_EINVAL, "materials: mats NULL/misaligned");
  if (bad4(scene->ref_nodes)) return fail(PTMI_EINVAL, "materials: ref_nodes NULL/misaligned");
  if (scene->n_inner > 0) {
    if (bad4(scene->nodes)) return fail(PTMI_EINVAL, "materials: nodes NULL/misaligned");
    if (bad4(slot)) return fail(PTMI_EINVAL, "materials: slot NULL/misaligned");
  }
  hipLaunchKernelGGL(mat_edit, dim3((unsigned)((n_edits + kMatBlock - 1) / kMatBlock)), dim3(kMatBlock), 0,
                     (hipStream_t)stream, s, q, t, const_cast<float*>(scene->mats),
                     const_cast<float*>(scene->ref_nodes), const_cast<float*>(scene->nodes), slot,
                     scene->num_bvh_nodes, scene->n_inner, scene->num_images);
  return hip_result(hipGetLastError());
}

}  // extern "C"
