// pt_edit_lists.hpp — what the ABIs that edit a resident scene in place share
// (pt_update.hip, pt_pose.hip, pt_material.hip). Each takes up to three edit
// lists (spheres, quads, triangles) of (device row, leaf node, payload) entries
// and runs one lane per entry:
//
//   * EditHead: the head of a list as a kernel argument. Each ABI's list type
//     (UpdList, PoseList, MatList) extends it with its own payload and says, for
//     the host half, how the payload is set and which of its pointers must be
//     4-byte aligned (set_payload, bad_payload).
//   * edit_select: a global lane index to (list, index within it).
//   * edit_target: THE SKIP RULE, stated here and nowhere else. An entry whose
//     ids are out of range, or whose leaf does not hold that primitive, names
//     nothing; the kernels store only behind this test.
//   * edit_fill, edit_check_pointers: the host half, with the messages the
//     three calls share, begun by the caller's prefix.
//   * upd_check_scene, upd_check_tree, upd_refit_launch: the refit step of the
//     update and the pose call (pt_update.hip defines them and owns the kernels).
//
// Nothing here tests which ABI is calling: the differences are the list types'.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ptmi_update.h"
#include "pt_args.hpp"
#include "pt_scene_rows.hpp"
#include "pt_update_math.hpp"

namespace ptmi {

constexpr int kEditBlock = 256;

struct EditHead {
  const int32_t* prim;
  const int32_t* leaf;
  int32_t count;
  int32_t num_prims;
  int32_t type;  // the type code of a leaf: 0 sphere, 1 triangle, 2 quad
};

// Lane i of the launch to its list `e` and its index in it; false past the last entry.
template <class L>
__device__ __forceinline__ bool edit_select(const L& s, const L& q, const L& t, L& e, int32_t& i) {
  e = s;
  if (i >= s.count) {
    i -= s.count;
    e = q;
    if (i >= q.count) {
      i -= q.count;
      e = t;
      if (i >= t.count) return false;
    }
  }
  return true;
}

// What entry i of a list names: the leaf's ref_nodes row, the primitive's device row and the leaf code.
struct EditTarget {
  float* ref;
  int32_t prim;
  uint32_t code;
};

// False, and nothing stored, unless prim is in [0, num_prims), leaf in
// [0, num_bvh_nodes) and the leaf's code names that primitive of that type.
__device__ __forceinline__ bool edit_target(const EditHead& e, int32_t i, float* ref_nodes, int32_t num_bvh_nodes,
                                            EditTarget& tg) {
  const int32_t p = e.prim[i], leaf = e.leaf[i];
  if (p < 0 || p >= e.num_prims || leaf < 0 || leaf >= num_bvh_nodes) return false;
  float* ref = ref_nodes + (size_t)leaf * kRefFloats;
  const uint32_t code = __float_as_uint(ref[kRefCode]);
  if (!leaf_code_names(code, e.type, p)) return false;
  tg = {ref, p, code};
  return true;
}

__device__ __forceinline__ void upd_store_box(float* ref, const UpdBox& b) {
  for (int k = 0; k < 3; ++k) {
    ref[k] = b.mn[k];
    ref[4 + k] = b.mx[k];
  }
}

// ---- the host half. Lists are in storage order: spheres, quads, triangles.
struct EditKind {
  const char* name;
  const char* count_name;
  int32_t type, row_floats;
};
constexpr EditKind kEditKinds[3] = {{"sphere", "num_spheres", 0, 4}, {"quad", "num_quads", 2, 16},
                                    {"triangle", "num_triangles", 1, 12}};

// d[k] from the ABI list abi[k] (NULL: empty) and the scene; `what` begins the message of a bad count.
// L::set_payload(abi list, kind k, the kind's primitive array, its first row of mats) sets the rest.
template <class L, class A>
int edit_fill(const char* what, const ptmi_scene_view* scene, const A* const (&abi)[3], L (&d)[3]) {
  const float* const prims[3] = {scene->spheres, scene->quads, scene->tris};
  const int32_t counts[3] = {scene->num_spheres, scene->num_quads, scene->num_triangles};
  int64_t base = 0;
  for (int k = 0; k < 3; ++k) {
    const A* a = abi[k];
    d[k].prim = a ? a->prim : nullptr;
    d[k].leaf = a ? a->leaf : nullptr;
    d[k].count = a ? a->count : 0;
    d[k].num_prims = counts[k];
    d[k].type = kEditKinds[k].type;
    d[k].set_payload(a, k, const_cast<float*>(prims[k]), (int32_t)base);
    if (d[k].count < 0 || d[k].count > counts[k])
      return fail(PTMI_EINVAL, "%s: %s count negative or above %s", what, kEditKinds[k].name,
                  kEditKinds[k].count_name);
    base += counts[k];
  }
  return PTMI_OK;
}

// The pointers of every non-empty list; `more(list, kind name)` is a list type's further check, run after each list's.
template <class L, class More>
int edit_check_pointers(const char* what, const L (&d)[3], More more) {
  for (int k = 0; k < 3; ++k) {
    if (d[k].count <= 0) continue;
    if (bad4(d[k].prim) || bad4(d[k].leaf) || d[k].bad_payload())
      return fail(PTMI_EINVAL, "%s: a %s list pointer is NULL/misaligned", what, kEditKinds[k].name);
    if (int rc = more(d[k], kEditKinds[k].name)) return rc;
  }
  return PTMI_OK;
}

template <class L>
int edit_check_pointers(const char* what, const L (&d)[3]) {
  return edit_check_pointers(what, d, [](const L&, const char*) { return (int)PTMI_OK; });
}

template <class L>
int64_t edit_total(const L (&d)[3]) {
  return (int64_t)d[0].count + d[1].count + d[2].count;
}

inline dim3 edit_grid(int64_t n_edits) { return dim3((unsigned)((n_edits + kEditBlock - 1) / kEditBlock)); }

// ---- the refit step of the update and the pose call
// The scene's counts checked; `what` ("update", "pose") begins the message.
int upd_check_scene(const ptmi_scene_view* scene, const char* what);

// ref_nodes, nodes, the topology and root_box checked for a call with n_edits
// edits in all: everything ptmi_update_primitives rejects after its lists.
int upd_check_tree(const ptmi_scene_view* scene, const ptmi_update_topology* topo, const float* root_box,
                   int64_t n_edits, const char* what);

// Step 2 and the root copy of a checked call, on `stream`. No HIP result is read.
void upd_refit_launch(const ptmi_scene_view* scene, const ptmi_update_topology* topo, float* root_box, void* stream);

}  // namespace ptmi
