/*
 * ptmi_update.h — the scene-update ABI of libptmi.so: primitives of a resident
 * scene are moved in place and the BVH above them is refitted on the device,
 * topology unchanged. It is versioned apart from PTMI_ABI_VERSION,
 * PTMI_POST_VERSION, PTMI_GUIDE_VERSION, PTMI_TEMPORAL_VERSION and
 * PTMI_WF_TILES_VERSION: nothing in ptmi.h, ptmi_post.h, ptmi_guide.h,
 * ptmi_temporal.h or ptmi_wf_tiles.h changes with it, and no render kernel is
 * involved. Error codes, ptmi_last_error(), ptmi_scene_view and the layouts of
 * nodes, ref_nodes, spheres, quads and tris are ptmi.h's.
 *
 * ---- What one call does, in this order
 *
 * Step 1, upd_leaves, one lane per edit of every list. Edit i of a list of
 * type T (sphere, quad, triangle) names
 *     prim[i]   the device primitive index (device order is leaf order),
 *     leaf[i]   the ref_nodes index of that primitive's leaf,
 *     row[i]    its new device row: 4, 16 or 12 f32 as ptmi.h lays them out,
 *     build[i]  its builder-form record, the form ptmi_bvh_build_sah takes:
 *               sphere 4 f32 {c.xyz, r}; quad 9 f32 {Q, u, v}; triangle 9 f32
 *               {v0, v1, v2} (v1 and v2 cannot be recovered from e1 and e2).
 * The lane copies row[i] over row prim[i] of the type's primitive array,
 * computes the leaf box from build[i] and writes it into min.xyz and max.xyz
 * of ref_nodes[leaf[i]]. The box is the builder's own f32 arithmetic, one
 * rounding per operation, no contraction, min(a, b) = (a < b) ? a : b and
 * max(a, b) = (a > b) ? a : b, per component k:
 *     sphere    mn = c - r; mx = c + r
 *     quad      c1 = Q + u; c2 = Q + v; c3 = (Q + u) + v;
 *               mn = min(min(min(Q, c1), c2), c3); mx likewise with max; pad
 *     triangle  mn = min(min(v0, v1), v2); mx likewise with max; pad
 *     pad       if (mx - mn < 0.0001f) { mid = (mn + mx) / 2.0f;
 *               mn = mid - 5e-05f; mx = mid + 5e-05f; }
 * Inputs are finite by contract. Ids within one list must be distinct. An edit
 * is skipped, and touches nothing, if prim[i] is outside [0, the type's
 * primitive count), if leaf[i] is outside [0, num_bvh_nodes), or if the leaf
 * code stored in ref_nodes[leaf[i]] does not name primitive prim[i] of type T.
 *
 * Step 2, upd_refit, for every level of internal nodes from the deepest up, one
 * launch per level on `stream`, one lane per internal node i of the level:
 *     l = left(i), r = right(i) of ref_nodes[i];
 *     ref_nodes[i].min = min(ref_nodes[l].min, ref_nodes[r].min), .max
 *     likewise with max (l is the first operand);
 *     row slot[i] of nodes: both children's boxes interleaved per component
 *     (f32 0 .. 11) and both centres (min + max) * 0.5f (f32 14 .. 19: z, x, y,
 *     child 0 then child 1); the two refs (f32 12, 13) are left alone.
 * Every internal node is refitted on every call, so boxes shrink as well as
 * grow. In a tree the builder made, every internal box already is this union
 * of its children's boxes, so a call without edits changes no byte, and an
 * edit followed by its inverse restores every byte. A node whose index, child
 * index or slot is out of range is skipped. One launch per level: the boundary
 * between dependent kernels on one stream is the ordering between a level and
 * the one above that needs no hand-off protocol between workgroups. With
 * PTMI_UPDATE_ONE_GROUP in the topology's flags the levels are walked by one
 * workgroup in one launch instead (below); the bits are the same.
 *
 * Root: min.xyz and max.xyz of ref_nodes[0] are then copied to root_box[0 .. 6)
 * (device memory). With n_inner == 0 only step 1 and this copy run; with
 * num_bvh_nodes == 0 nothing runs.
 *
 * ---- Topology, made once per scene by the host
 *
 *     order      device int32[n_inner]: the ref_nodes indices of the internal
 *                nodes, deepest level first;
 *     level_end  HOST int32[n_levels]: level j is order[level_end[j-1] ..
 *                level_end[j]) (from 0 for j = 0); strictly ascending, the last
 *                equal to n_inner; read during the call only;
 *     slot       device int32[num_bvh_nodes]: the row in nodes of each internal
 *                node, -1 for leaves.
 *
 * ---- Call semantics
 *
 * Asynchronous on `stream`; no allocation; not timed by ptmi_prof_*. The call
 * WRITES through the scene view's nodes, ref_nodes, spheres, quads and tris
 * pointers, although the view declares them const: the caller must have no
 * render (or any other reader) of this scene in flight on another stream, and
 * orders later renders after the call as after any work on `stream`. The view's
 * host fields (root_min, root_max, shell) are the caller's to refresh: the root
 * box from root_box; the shell hint is a claim about the boxes (ptmi.h) that an
 * update can break, and 0 is always valid.
 */
#ifndef PTMI_UPDATE_H
#define PTMI_UPDATE_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_UPDATE_VERSION 1

/* The edits of one primitive type: device pointers, count entries each. */
typedef struct ptmi_update_list {
    const int32_t *prim;
    const int32_t *leaf;
    const float *row;      /* count x 4 / 16 / 12 f32 (sphere / quad / triangle) */
    const float *build;    /* count x 4 / 9 / 9 f32 */
    int32_t count;
} ptmi_update_list;

/* flags of ptmi_update_topology: the single-workgroup form of step 2. One
 * launch of one 1024-lane workgroup walks the levels itself behind
 * __syncthreads() (its waves share one CU and its L1, so a level's stores are
 * seen by the next level's loads); the same bits. At most
 * PTMI_UPDATE_ONE_GROUP_MAX_LEVELS levels. */
#define PTMI_UPDATE_ONE_GROUP 1
#define PTMI_UPDATE_ONE_GROUP_MAX_LEVELS 64

typedef struct ptmi_update_topology {
    const int32_t *order;      /* device */
    const int32_t *slot;       /* device */
    const int32_t *level_end;  /* host */
    int32_t n_levels;
    int32_t flags;             /* 0, or PTMI_UPDATE_ONE_GROUP */
} ptmi_update_topology;

/* Applies the edits and refits (see above). A NULL list is a list of count 0;
 * all counts zero is a pure refit. PTMI_EINVAL, each with a message and before
 * any HIP call: a NULL scene; a negative count or one above the type's
 * primitive count; a NULL or misaligned (4 B) pointer of a list with count > 0; NULL
 * ref_nodes while n_inner > 0 or a count > 0; NULL nodes, topo, order, slot,
 * level_end or root_box while n_inner > 0; n_levels < 1 or level ends that are
 * not strictly ascending from above 0 to n_inner; flags other than
 * PTMI_UPDATE_ONE_GROUP, or that flag with more than
 * PTMI_UPDATE_ONE_GROUP_MAX_LEVELS levels. */
int ptmi_update_primitives(const ptmi_scene_view *scene, const ptmi_update_list *spheres,
                           const ptmi_update_list *quads, const ptmi_update_list *tris,
                           const ptmi_update_topology *topo, float *root_box, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_UPDATE_H */
