// pt_pose.hip — the pose ABI (include/ptmi_pose.h): tracked primitives put
// where they are at a shutter time t and the BVH refitted above them
// (DESIGN.md §24).
//
//   * pose_leaves: one lane per track entry of the three lists: the points are
//     p + t * d in f64, cast to f32; the lane writes the row floats that change
//     and the leaf box into ref_nodes. An entry whose ids are out of range, or
//     whose leaf does not hold that primitive, is skipped, as upd_leaves does.
//   * the refit and the root copy are pt_update.hip's kernels, launched through
//     pt_update_launch.hpp.
//
// The arithmetic is pt_pose_math.hpp's, shared with pose_check.cpp; the box
// rules are pt_update_math.hpp's. A few thousand lanes at most: no LDS, no
// cross-lane reads, nothing timed by ptmi_prof_*. No render kernel is involved.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ptmi_pose.h"
#include "pt_args.hpp"
#include "pt_pose_math.hpp"
#include "pt_update_launch.hpp"

namespace ptmi {

constexpr int kPoseBlock = 256;
constexpr int kPoseRefFloats = 12;  // a ref_nodes row (include/ptmi.h)

// One list of tracks as a kernel argument, with what its type fixes.
struct PoseList {
  const int32_t* prim;
  const int32_t* leaf;
  const double* rec;
  float* prims;  // the type's primitive array
  int32_t count;
  int32_t num_prims;
  int32_t type;  // the type code of a leaf: 0 sphere, 1 triangle, 2 quad
  int32_t row_floats, rec_doubles;
};

__global__ __launch_bounds__(kPoseBlock) void pose_leaves(PoseList s, PoseList q, PoseList t, double time,
                                                          float* __restrict__ ref_nodes, int32_t num_bvh_nodes) {
  int32_t i = (int32_t)(blockIdx.x * (uint32_t)kPoseBlock + threadIdx.x);
  PoseList e = s;
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
  float* ref = ref_nodes + (size_t)leaf * kPoseRefFloats;
  // leaf code 0x80000000 | type << 28 | class << 25 | index: this primitive's leaf?
  const uint32_t code = __float_as_uint(ref[9]);
  if ((code >> 28) != (8u | (uint32_t)e.type) || (code & 0x1ffffffu) != (uint32_t)p) return;
  const double* rec = e.rec + (size_t)i * e.rec_doubles;
  float* row = e.prims + (size_t)p * e.row_floats;
  const UpdBox box = e.type == 0 ? pose_sphere(rec, time, row)
                     : e.type == 2 ? pose_quad(rec, time, row)
                                   : pose_tri(rec, time, row);
  for (int k = 0; k < 3; ++k) {
    ref[k] = box.mn[k];
    ref[4 + k] = box.mx[k];
  }
}

static bool pose_fill(PoseList& d, const ptmi_pose_list* s, const float* prims, int32_t num_prims, int32_t type,
                      int32_t row_floats, int32_t rec_doubles) {
  d.prim = s ? s->prim : nullptr;
  d.leaf = s ? s->leaf : nullptr;
  d.rec = s ? s->rec : nullptr;
  d.prims = const_cast<float*>(prims);
  d.count = s ? s->count : 0;
  d.num_prims = num_prims;
  d.type = type;
  d.row_floats = row_floats;
  d.rec_doubles = rec_doubles;
  return d.count >= 0 && d.count <= num_prims;
}

inline bool bad8(const void* p) { return !p || ((uintptr_t)p & 7u); }

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_pose_primitives(const ptmi_scene_view* scene, const ptmi_pose_list* spheres, const ptmi_pose_list* quads,
                         const ptmi_pose_list* tris, double t, const ptmi_update_topology* topo, float* root_box,
                         void* stream) {
  if (int rc = upd_check_scene(scene, "pose")) return rc;
  if (!std::isfinite(t)) return fail(PTMI_EINVAL, "pose: t is not finite");
  PoseList s, q, r;
  if (!pose_fill(s, spheres, scene->spheres, scene->num_spheres, 0, 4, 6))
    return fail(PTMI_EINVAL, "pose: sphere count negative or above num_spheres");
  if (!pose_fill(q, quads, scene->quads, scene->num_quads, 2, 16, 9))
    return fail(PTMI_EINVAL, "pose: quad count negative or above num_quads");
  if (!pose_fill(r, tris, scene->tris, scene->num_triangles, 1, 12, 12))
    return fail(PTMI_EINVAL, "pose: triangle count negative or above num_triangles");
  const struct {
    const PoseList& l;
    const char* name;
  } lists[3] = {{s, "sphere"}, {q, "quad"}, {r, "triangle"}};
  for (const auto& e : lists) {
    if (e.l.count <= 0) continue;
    if (bad4(e.l.prim) || bad4(e.l.leaf) || bad4(e.l.prims))
      return fail(PTMI_EINVAL, "pose: a %s list pointer is NULL/misaligned", e.name);
    if (bad8(e.l.rec)) return fail(PTMI_EINVAL, "pose: a %s list's rec is NULL or not 8-byte aligned", e.name);
  }
  const int64_t n_tracks = (int64_t)s.count + q.count + r.count;
  if (int rc = upd_check_tree(scene, topo, root_box, n_tracks, "pose")) return rc;
  if (scene->num_bvh_nodes == 0) return PTMI_OK;
  if (n_tracks > 0)
    hipLaunchKernelGGL(pose_leaves, dim3((unsigned)((n_tracks + kPoseBlock - 1) / kPoseBlock)), dim3(kPoseBlock), 0,
                       (hipStream_t)stream, s, q, r, t, const_cast<float*>(scene->ref_nodes), scene->num_bvh_nodes);
  upd_refit_launch(scene, topo, root_box, stream);
  return hip_result(hipGetLastError());
}

}  // extern "C"
