// pt_material.hip — the material-edit ABI (include/ptmi_material.h): mats rows
// of a resident scene replaced in place, and the leaf codes that carry each
// primitive's material class patched with them.
//
//   * mat_edit: one lane per edit of the three lists: the 20-f32 row is copied
//     over the primitive's mats row, the class of its new flags word replaces
//     the class bits of the leaf code in ref_nodes (the stackless traversal's
//     copy) and in the parent's nodes row (the stack traversal's). An edit
//     whose ids are out of range, whose leaf does not hold that primitive
//     (pt_edit_lists.hpp's skip rule, shared with upd_leaves and pose_leaves) or
//     whose flags name an image the scene does not have is skipped.
//
// The integer rules are pt_material_math.hpp's and pt_scene_rows.hpp's, shared
// with material_check.cpp. A few thousand lanes of loads and vector stores: no
// LDS, no cross-lane reads, nothing timed by ptmi_prof_*. No render kernel is
// involved.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_material.h"
#include "pt_edit_lists.hpp"
#include "pt_material_math.hpp"

namespace ptmi {

// One list of edits as a kernel argument, with what its type fixes.
struct MatList : EditHead {
  const float* row;
  int32_t base;  // the type's first row of mats (storage order: spheres, quads, triangles)

  void set_payload(const ptmi_material_list* a, int, float*, int32_t first_row) {
    row = a ? a->row : nullptr;
    base = first_row;
  }
  bool bad_payload() const { return bad4(row); }
};

__global__ __launch_bounds__(kEditBlock) void mat_edit(MatList s, MatList q, MatList t, float* __restrict__ mats,
                                                       float* __restrict__ ref_nodes, float* __restrict__ nodes,
                                                       const int32_t* __restrict__ slot, int32_t num_bvh_nodes,
                                                       int32_t n_inner, int32_t num_images) {
  int32_t i = (int32_t)(blockIdx.x * (uint32_t)kEditBlock + threadIdx.x);
  MatList e;
  EditTarget tg;
  if (!edit_select(s, q, t, e, i) || !edit_target(e, i, ref_nodes, num_bvh_nodes, tg)) return;
  const float* row = e.row + (size_t)i * kMatFloats;
  const uint32_t flags = __float_as_uint(row[kMatFloats - 1]);
  if (!mat_image_ok(flags, num_images)) return;
  float* dst = mats + ((size_t)e.base + (size_t)tg.prim) * kMatFloats;
  for (int k = 0; k < kMatFloats; ++k) dst[k] = row[k];
  const float patched = __uint_as_float(leaf_patch_class(tg.code, mat_class(flags)));
  const int32_t parent = __float_as_int(tg.ref[8]), side = __float_as_int(tg.ref[10]);
  tg.ref[kRefCode] = patched;
  // the stack traversal's copy: child ref `side` of the parent's nodes row; the root has none
  if (n_inner <= 0 || parent < 0 || parent >= num_bvh_nodes || (side != 0 && side != 1)) return;
  const int32_t sl = slot[parent];
  if (sl < 0 || sl >= n_inner) return;
  nodes[(size_t)sl * kNodeFloats + 12 + side] = patched;
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
  MatList l[3];
  const ptmi_material_list* const abi[3] = {spheres, quads, tris};
  if (int rc = edit_fill("materials", scene, abi, l)) return rc;
  if (int rc = edit_check_pointers("materials", l)) return rc;
  const int64_t n_edits = edit_total(l);
  if (n_edits == 0) return PTMI_OK;
  if (bad4(scene->mats)) return fail(PTMI_EINVAL, "materials: mats NULL/misaligned");
  if (bad4(scene->ref_nodes)) return fail(PTMI_EINVAL, "materials: ref_nodes NULL/misaligned");
  if (scene->n_inner > 0) {
    if (bad4(scene->nodes)) return fail(PTMI_EINVAL, "materials: nodes NULL/misaligned");
    if (bad4(slot)) return fail(PTMI_EINVAL, "materials: slot NULL/misaligned");
  }
  hipLaunchKernelGGL(mat_edit, edit_grid(n_edits), dim3(kEditBlock), 0, (hipStream_t)stream, l[0], l[1], l[2],
                     const_cast<float*>(scene->mats), const_cast<float*>(scene->ref_nodes),
                     const_cast<float*>(scene->nodes), slot, scene->num_bvh_nodes, scene->n_inner, scene->num_images);
  return hip_result(hipGetLastError());
}

}  // extern "C"
