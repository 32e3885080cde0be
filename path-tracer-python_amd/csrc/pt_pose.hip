// pt_pose.hip — the pose ABI (include/ptmi_pose.h): tracked primitives put
// where they are at a shutter time t and the BVH refitted above them
// (DESIGN.md §24).
//
//   * pose_leaves: one lane per track entry of the three lists: the points are
//     p + t * d in f64, cast to f32; the lane writes the row floats that change
//     and the leaf box into ref_nodes. An entry whose ids are out of range, or
//     whose leaf does not hold that primitive, is skipped, as upd_leaves does:
//     the lists' head, the selection and the skip rule are pt_edit_lists.hpp's.
//   * the refit and the root copy are pt_update.hip's kernels, launched through
//     the functions pt_edit_lists.hpp declares.
//
// The arithmetic is pt_pose_math.hpp's, shared with pose_check.cpp; the box
// rules are pt_update_math.hpp's. A few thousand lanes at most: no LDS, no
// cross-lane reads, nothing timed by ptmi_prof_*. No render kernel is involved.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ptmi_pose.h"
#include "pt_edit_lists.hpp"
#include "pt_pose_math.hpp"

namespace ptmi {

// One list of tracks as a kernel argument, with what its type fixes.
struct PoseList : EditHead {
  const double* rec;
  float* prims;  // the type's primitive array
  int32_t row_floats, rec_doubles;

  void set_payload(const ptmi_pose_list* a, int k, float* rows, int32_t) {
    rec = a ? a->rec : nullptr;
    prims = rows;
    row_floats = kEditKinds[k].row_floats;
    rec_doubles = 6 + 3 * k;  // sphere {o, d}, quad {Q, d, normal}, triangle {v0, v1, v2, d}
  }
  bool bad_payload() const { return bad4(prims); }  // rec has its own message
};

__global__ __launch_bounds__(kEditBlock) void pose_leaves(PoseList s, PoseList q, PoseList t, double time,
                                                          float* __restrict__ ref_nodes, int32_t num_bvh_nodes) {
  int32_t i = (int32_t)(blockIdx.x * (uint32_t)kEditBlock + threadIdx.x);
  PoseList e;
  EditTarget tg;
  if (!edit_select(s, q, t, e, i) || !edit_target(e, i, ref_nodes, num_bvh_nodes, tg)) return;
  const double* rec = e.rec + (size_t)i * e.rec_doubles;
  float* row = e.prims + (size_t)tg.prim * e.row_floats;
  const UpdBox box = e.type == 0 ? pose_sphere(rec, time, row)
                     : e.type == 2 ? pose_quad(rec, time, row)
                                   : pose_tri(rec, time, row);
  upd_store_box(tg.ref, box);
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_pose_primitives(const ptmi_scene_view* scene, const ptmi_pose_list* spheres, const ptmi_pose_list* quads,
                         const ptmi_pose_list* tris, double t, const ptmi_update_topology* topo, float* root_box,
                         void* stream) {
  if (int rc = upd_check_scene(scene, "pose")) return rc;
  if (!std::isfinite(t)) return fail(PTMI_EINVAL, "pose: t is not finite");
  PoseList l[3];
  const ptmi_pose_list* const abi[3] = {spheres, quads, tris};
  if (int rc = edit_fill("pose", scene, abi, l)) return rc;
  const auto rec_aligned = [](const PoseList& e, const char* kind) {
    return bad8(e.rec) ? fail(PTMI_EINVAL, "pose: a %s list's rec is NULL or not 8-byte aligned", kind) : (int)PTMI_OK;
  };
  if (int rc = edit_check_pointers("pose", l, rec_aligned)) return rc;
  const int64_t n_tracks = edit_total(l);
  if (int rc = upd_check_tree(scene, topo, root_box, n_tracks, "pose")) return rc;
  if (scene->num_bvh_nodes == 0) return PTMI_OK;
  if (n_tracks > 0)
    hipLaunchKernelGGL(pose_leaves, edit_grid(n_tracks), dim3(kEditBlock), 0, (hipStream_t)stream, l[0], l[1], l[2], t,
                       const_cast<float*>(scene->ref_nodes), scene->num_bvh_nodes);
  upd_refit_launch(scene, topo, root_box, stream);
  return hip_result(hipGetLastError());
}

}  // extern "C"
