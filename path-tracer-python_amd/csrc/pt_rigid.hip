// pt_rigid.hip — the rigid-body pose ABI (include/ptmi_rigid.h): the primitives
// of bodies put where the bodies' transforms at one time take them and the BVH
// refitted above them.
//
//   * rigid_leaves: one lane per entry of the three lists: the lane reads its
//     body's 15 doubles from the table in the kernel arguments, transforms the
//     entry's f64 rest record, casts to f32, writes the row floats and the leaf
//     box into ref_nodes. An entry whose ids are out of range, or whose leaf
//     does not hold that primitive, is skipped, as upd_leaves does (the lists'
//     head, the selection and the skip rule are pt_edit_lists.hpp's), and so is
//     one whose body index is outside the table.
//   * the refit and the root copy are pt_update.hip's kernels, launched through
//     the functions pt_edit_lists.hpp declares.
//
// The arithmetic is pt_rigid_math.hpp's, shared with rigid_check.cpp; the box
// rules are pt_update_math.hpp's. A few thousand lanes at most: no LDS, no
// cross-lane reads, nothing timed by ptmi_prof_*. No render kernel is involved.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ptmi_rigid.h"
#include "pt_edit_lists.hpp"
#include "pt_rigid_math.hpp"

namespace ptmi {

static_assert(sizeof(ptmi_rigid_body) == kRigidBodyDoubles * sizeof(double), "a body is 15 packed doubles");

// One list of entries as a kernel argument, with what its type fixes.
struct RigidList : EditHead {
  const double* rec;
  const int32_t* body;
  float* prims;  // the type's primitive array
  int32_t row_floats, rec_doubles;

  void set_payload(const ptmi_rigid_list* a, int k, float* rows, int32_t) {
    rec = a ? a->rec : nullptr;
    body = a ? a->body : nullptr;
    prims = rows;
    row_floats = kEditKinds[k].row_floats;
    rec_doubles = k == 0 ? 3 : k == 1 ? 15 : 18;  // sphere {c}, quad {Q, u, v, normal, w}, triangle {v0, v1, v2, e1, e2, n}
  }
  bool bad_payload() const { return bad4(prims); }  // rec and body have their own messages
};

// The body table, by value in the kernel arguments: 1920 B.
struct RigidBodies {
  ptmi_rigid_body b[PTMI_RIGID_MAX_BODIES];
};

__global__ __launch_bounds__(kEditBlock) void rigid_leaves(RigidList s, RigidList q, RigidList t, RigidBodies bodies,
                                                           int32_t n_bodies, float* __restrict__ ref_nodes,
                                                           int32_t num_bvh_nodes) {
  int32_t i = (int32_t)(blockIdx.x * (uint32_t)kEditBlock + threadIdx.x);
  RigidList e;
  EditTarget tg;
  if (!edit_select(s, q, t, e, i) || !edit_target(e, i, ref_nodes, num_bvh_nodes, tg)) return;
  const int32_t bi = e.body[i];
  if (bi < 0 || bi >= n_bodies) return;
  const double* body = bodies.b[bi].R;  // R, pivot, pivot_t: 15 doubles in a row
  const double* rec = e.rec + (size_t)i * e.rec_doubles;
  float* row = e.prims + (size_t)tg.prim * e.row_floats;
  const UpdBox box = e.type == 0 ? rigid_sphere(rec, body, row)
                     : e.type == 2 ? rigid_quad(rec, body, row)
                                   : rigid_tri(rec, body, row);
  upd_store_box(tg.ref, box);
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_pose_rigid(const ptmi_scene_view* scene, const ptmi_rigid_list* spheres, const ptmi_rigid_list* quads,
                    const ptmi_rigid_list* tris, const ptmi_rigid_body* bodies, int32_t n_bodies,
                    const ptmi_update_topology* topo, float* root_box, void* stream) {
  if (int rc = upd_check_scene(scene, "rigid")) return rc;
  if (n_bodies < 0 || n_bodies > PTMI_RIGID_MAX_BODIES)
    return fail(PTMI_EINVAL, "rigid: n_bodies outside [0, %d]", PTMI_RIGID_MAX_BODIES);
  if (n_bodies > 0 && !bodies) return fail(PTMI_EINVAL, "rigid: bodies is NULL");
  RigidBodies table = {};
  for (int32_t b = 0; b < n_bodies; ++b) {
    table.b[b] = bodies[b];
    const double* v = table.b[b].R;
    for (int k = 0; k < kRigidBodyDoubles; ++k)
      if (!std::isfinite(v[k])) return fail(PTMI_EINVAL, "rigid: body %d has a value that is not finite", (int)b);
  }
  RigidList l[3];
  const ptmi_rigid_list* const abi[3] = {spheres, quads, tris};
  if (int rc = edit_fill("rigid", scene, abi, l)) return rc;
  const auto more = [](const RigidList& e, const char* kind) {
    if (bad8(e.rec)) return fail(PTMI_EINVAL, "rigid: a %s list's rec is NULL or not 8-byte aligned", kind);
    if (bad4(e.body)) return fail(PTMI_EINVAL, "rigid: a %s list's body is NULL or not 4-byte aligned", kind);
    return (int)PTMI_OK;
  };
  if (int rc = edit_check_pointers("rigid", l, more)) return rc;
  const int64_t n_entries = edit_total(l);
  if (int rc = upd_check_tree(scene, topo, root_box, n_entries, "rigid")) return rc;
  if (scene->num_bvh_nodes == 0) return PTMI_OK;
  if (n_entries > 0)
    hipLaunchKernelGGL(rigid_leaves, edit_grid(n_entries), dim3(kEditBlock), 0, (hipStream_t)stream, l[0], l[1], l[2],
                       table, n_bodies, const_cast<float*>(scene->ref_nodes), scene->num_bvh_nodes);
  upd_refit_launch(scene, topo, root_box, stream);
  return hip_result(hipGetLastError());
}

}  // extern "C"
