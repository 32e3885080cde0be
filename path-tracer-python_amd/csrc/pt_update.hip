// pt_update.hip — the scene-update ABI (include/ptmi_update.h): primitives
// moved in place and the BVH refitted above them.
//
//   * upd_leaves: one lane per edit of the three lists: the primitive row is
//     copied and the leaf box, computed from the builder-form record, is
//     written into ref_nodes. An edit whose ids are out of range, or whose leaf
//     does not hold that primitive, is skipped.
//   * upd_refit: one launch per level of internal nodes, deepest first, one
//     lane per node: the union of the two children's boxes goes to ref_nodes
//     and both children's boxes and centres go to the node's 80-B row. The
//     levels are ordered by the kernel boundary on the stream: the per-XCD L2s
//     are not coherent with each other within a launch, so a level written by
//     one launch is read by the next and by no lane of its own.
//   * upd_refit_one (PTMI_UPDATE_ONE_GROUP): the same refit as one launch of
//     one 1024-lane workgroup that walks the levels behind __syncthreads();
//     faster on trees of a few thousand nodes, chosen by the caller.
//   * upd_root: ref_nodes[0]'s box to the caller's float[6].
//
// The lists' head, the selection of a lane's entry, the skip rule and the
// host checks of the lists are pt_edit_lists.hpp's, shared with the pose and
// the material ABI (pt_pose.hip, pt_material.hip). The scene and topology
// checks and the launches of the refit and the root copy are declared there
// too: the pose ABI runs the same step 2 after its own step 1.
//
// The arithmetic is pt_update_math.hpp's, shared with update_check.cpp. A few
// thousand lanes of min / max: no LDS, no cross-lane reads, nothing timed by
// ptmi_prof_*. No render kernel is involved.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_update.h"
#include "pt_edit_lists.hpp"

namespace ptmi {

constexpr int kUpdBlock = 256;

// One list of edits as a kernel argument, with what its type fixes.
struct UpdList : EditHead {
  const float* row;
  const float* build;
  float* prims;  // the type's primitive array
  int32_t row_floats, build_floats;

  void set_payload(const ptmi_update_list* a, int k, float* rows, int32_t) {
    row = a ? a->row : nullptr;
    build = a ? a->build : nullptr;
    prims = rows;
    row_floats = kEditKinds[k].row_floats;
    build_floats = k == 0 ? 4 : 9;
  }
  bool bad_payload() const { return bad4(row) || bad4(build) || bad4(prims); }
};

__device__ __forceinline__ UpdBox upd_load_box(const float* ref) {
  UpdBox b;
  for (int k = 0; k < 3; ++k) {
    b.mn[k] = ref[k];
    b.mx[k] = ref[4 + k];
  }
  return b;
}

__global__ __launch_bounds__(kEditBlock) void upd_leaves(UpdList s, UpdList q, UpdList t, float* __restrict__ ref_nodes,
                                                         int32_t num_bvh_nodes) {
  int32_t i = (int32_t)(blockIdx.x * (uint32_t)kEditBlock + threadIdx.x);
  UpdList e;
  EditTarget tg;
  if (!edit_select(s, q, t, e, i) || !edit_target(e, i, ref_nodes, num_bvh_nodes, tg)) return;
  const float* row = e.row + (size_t)i * e.row_floats;
  float* dst = e.prims + (size_t)tg.prim * e.row_floats;
  for (int k = 0; k < e.row_floats; ++k) dst[k] = row[k];
  const float* rec = e.build + (size_t)i * e.build_floats;
  float b9[9];
  for (int k = 0; k < 9; ++k) b9[k] = (k < e.build_floats) ? rec[k] : 0.0f;
  const UpdBox box = e.type == 0 ? upd_sphere_box(b9) : e.type == 2 ? upd_quad_box(b9) : upd_tri_box(b9);
  upd_store_box(tg.ref, box);
}

// Internal node i: the union of its children's boxes into ref_nodes[i], their
// boxes and centres into row slot[i] of nodes.
__device__ __forceinline__ void upd_refit_node(int32_t i, const int32_t* __restrict__ slot, float* ref_nodes,
                                               float* __restrict__ nodes, int32_t num_bvh_nodes, int32_t n_inner) {
  if (i < 0 || i >= num_bvh_nodes) return;
  float* ref = ref_nodes + (size_t)i * kRefFloats;
  const int32_t l = __float_as_int(ref[3]), r = __float_as_int(ref[7]), sl = slot[i];
  if (l < 0 || l >= num_bvh_nodes || r < 0 || r >= num_bvh_nodes || sl < 0 || sl >= n_inner) return;
  const UpdBox bl = upd_load_box(ref_nodes + (size_t)l * kRefFloats);
  const UpdBox br = upd_load_box(ref_nodes + (size_t)r * kRefFloats);
  upd_store_box(ref, upd_union(bl, br));
  float4* row = (float4*)(nodes + (size_t)sl * kNodeFloats);  // 80-B rows of a 16-B aligned array
  row[0] = make_float4(bl.mn[0], br.mn[0], bl.mn[1], br.mn[1]);
  row[1] = make_float4(bl.mn[2], br.mn[2], bl.mx[0], br.mx[0]);
  row[2] = make_float4(bl.mx[1], br.mx[1], bl.mx[2], br.mx[2]);
  ((float2*)row)[7] = make_float2(upd_centre(bl, 2), upd_centre(br, 2));  // f32 14, 15; 12 and 13 are the refs
  row[4] = make_float4(upd_centre(bl, 0), upd_centre(br, 0), upd_centre(bl, 1), upd_centre(br, 1));
}

__global__ __launch_bounds__(kUpdBlock) void upd_refit(const int32_t* __restrict__ order, int32_t begin, int32_t end,
                                                       const int32_t* __restrict__ slot, float* ref_nodes,
                                                       float* __restrict__ nodes, int32_t num_bvh_nodes,
                                                       int32_t n_inner) {
  const int32_t j = begin + (int32_t)(blockIdx.x * (uint32_t)kUpdBlock + threadIdx.x);
  if (j >= end) return;
  upd_refit_node(order[j], slot, ref_nodes, nodes, num_bvh_nodes, n_inner);
}

// The single-workgroup form (PTMI_UPDATE_ONE_GROUP): one block walks the levels
// itself. All its waves share one CU and its vector L1, so a level's stores are
// visible to the next level's loads behind __syncthreads(); the level ends are a
// kernel argument, so every wave runs the same number of barriers.
constexpr int kUpdOneBlock = 1024;
struct UpdLevels {
  int32_t n;
  int32_t end[PTMI_UPDATE_ONE_GROUP_MAX_LEVELS];
};

__global__ __launch_bounds__(kUpdOneBlock) void upd_refit_one(const int32_t* __restrict__ order, UpdLevels lv,
                                                              const int32_t* __restrict__ slot, float* ref_nodes,
                                                              float* __restrict__ nodes, int32_t num_bvh_nodes,
                                                              int32_t n_inner) {
  int32_t begin = 0;
  for (int32_t j = 0; j < lv.n; ++j) {
    const int32_t end = lv.end[j];
    for (int32_t k = begin + (int32_t)threadIdx.x; k < end; k += kUpdOneBlock)
      upd_refit_node(order[k], slot, ref_nodes, nodes, num_bvh_nodes, n_inner);
    begin = end;
    __syncthreads();
  }
}

__global__ void upd_root(const float* __restrict__ ref_nodes, float* __restrict__ root_box) {
  const int k = (int)threadIdx.x;
  if (k < 6) root_box[k] = ref_nodes[k < 3 ? k : k + 1];
}

// ---- the refit step shared with the pose ABI (pt_edit_lists.hpp)
int upd_check_scene(const ptmi_scene_view* scene, const char* what) {
  if (!scene) return fail(PTMI_EINVAL, "%s: scene is NULL", what);
  if (scene->n_inner < 0 || scene->num_bvh_nodes < 0 || scene->num_spheres < 0 || scene->num_quads < 0 ||
      scene->num_triangles < 0 || (scene->n_inner > 0 && scene->num_bvh_nodes != 2 * scene->n_inner + 1))
    return fail(PTMI_EINVAL, "%s: bad scene counts (num_bvh_nodes must be 2 * n_inner + 1)", what);
  return PTMI_OK;
}

int upd_check_tree(const ptmi_scene_view* scene, const ptmi_update_topology* topo, const float* root_box,
                   int64_t n_edits, const char* what) {
  const int32_t n_inner = scene->n_inner;
  if ((n_inner > 0 || n_edits > 0) && bad4(scene->ref_nodes))
    return fail(PTMI_EINVAL, "%s: ref_nodes NULL/misaligned", what);
  if (n_inner > 0) {
    if (bad16(scene->nodes)) return fail(PTMI_EINVAL, "%s: nodes NULL/misaligned", what);
    if (!topo) return fail(PTMI_EINVAL, "%s: topo is NULL", what);
    if (bad4(topo->order)) return fail(PTMI_EINVAL, "%s: order NULL/misaligned", what);
    if (bad4(topo->slot)) return fail(PTMI_EINVAL, "%s: slot NULL/misaligned", what);
    if (bad4(root_box)) return fail(PTMI_EINVAL, "%s: root_box NULL/misaligned", what);
    if (!topo->level_end || topo->n_levels < 1)
      return fail(PTMI_EINVAL, "%s: level_end is NULL or n_levels < 1", what);
    int32_t prev = 0;
    for (int32_t j = 0; j < topo->n_levels; ++j) {
      if (topo->level_end[j] <= prev || topo->level_end[j] > n_inner)
        return fail(PTMI_EINVAL, "%s: level ends must ascend strictly to n_inner", what);
      prev = topo->level_end[j];
    }
    if (prev != n_inner) return fail(PTMI_EINVAL, "%s: level ends must ascend strictly to n_inner", what);
    if (topo->flags & ~PTMI_UPDATE_ONE_GROUP) return fail(PTMI_EINVAL, "%s: unknown flags", what);
    if ((topo->flags & PTMI_UPDATE_ONE_GROUP) && topo->n_levels > PTMI_UPDATE_ONE_GROUP_MAX_LEVELS)
      return fail(PTMI_EINVAL, "%s: too many levels for PTMI_UPDATE_ONE_GROUP", what);
  }
  return PTMI_OK;
}

void upd_refit_launch(const ptmi_scene_view* scene, const ptmi_update_topology* topo, float* root_box, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int32_t n_inner = scene->n_inner;
  float* ref_nodes = const_cast<float*>(scene->ref_nodes);
  if (n_inner > 0 && (topo->flags & PTMI_UPDATE_ONE_GROUP)) {
    UpdLevels lv;
    lv.n = topo->n_levels;
    for (int32_t j = 0; j < topo->n_levels; ++j) lv.end[j] = topo->level_end[j];
    hipLaunchKernelGGL(upd_refit_one, dim3(1), dim3(kUpdOneBlock), 0, st, topo->order, lv, topo->slot, ref_nodes,
                       const_cast<float*>(scene->nodes), scene->num_bvh_nodes, n_inner);
  } else if (n_inner > 0) {
    int32_t begin = 0;
    for (int32_t j = 0; j < topo->n_levels; ++j) {
      const int32_t end = topo->level_end[j];
      hipLaunchKernelGGL(upd_refit, dim3((unsigned)((end - begin + kUpdBlock - 1) / kUpdBlock)), dim3(kUpdBlock), 0, st,
                         topo->order, begin, end, topo->slot, ref_nodes, const_cast<float*>(scene->nodes),
                         scene->num_bvh_nodes, n_inner);
      begin = end;
    }
  }
  if (root_box && ref_nodes) hipLaunchKernelGGL(upd_root, dim3(1), dim3(64), 0, st, ref_nodes, root_box);
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_update_primitives(const ptmi_scene_view* scene, const ptmi_update_list* spheres,
                           const ptmi_update_list* quads, const ptmi_update_list* tris,
                           const ptmi_update_topology* topo, float* root_box, void* stream) {
  if (int rc = upd_check_scene(scene, "update")) return rc;
  UpdList l[3];
  const ptmi_update_list* const abi[3] = {spheres, quads, tris};
  if (int rc = edit_fill("update", scene, abi, l)) return rc;
  if (int rc = edit_check_pointers("update", l)) return rc;
  const int64_t n_edits = edit_total(l);
  if (int rc = upd_check_tree(scene, topo, root_box, n_edits, "update")) return rc;
  if (scene->num_bvh_nodes == 0) return PTMI_OK;
  if (n_edits > 0)
    hipLaunchKernelGGL(upd_leaves, edit_grid(n_edits), dim3(kEditBlock), 0, (hipStream_t)stream, l[0], l[1], l[2],
                       const_cast<float*>(scene->ref_nodes), scene->num_bvh_nodes);
  upd_refit_launch(scene, topo, root_box, stream);
  return hip_result(hipGetLastError());
}

}  // extern "C"
