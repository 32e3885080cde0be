/*
 * ptmi_tree.h — the tree-quality ABI of libptmi.so: how far the boxes of a
 * refitted BVH (ptmi_update.h) have grown since the tree was built, measured on
 * the device, and the id-image remap that carries a motion-aware history
 * (ptmi_motion.h) across a rebuild of the resident scene. It is versioned apart
 * from PTMI_ABI_VERSION, PTMI_POST_VERSION, PTMI_GUIDE_VERSION,
 * PTMI_TEMPORAL_VERSION, PTMI_WF_TILES_VERSION, PTMI_UPDATE_VERSION and
 * PTMI_MOTION_VERSION: nothing in ptmi.h, ptmi_post.h, ptmi_guide.h,
 * ptmi_temporal.h, ptmi_wf_tiles.h, ptmi_update.h or ptmi_motion.h changes with
 * it, and no render kernel is involved. Error codes, ptmi_last_error(),
 * ptmi_scene_view and the layout of ref_nodes are ptmi.h's; the id image is
 * ptmi_motion.h's.
 *
 * ---- The figure
 *
 * The surface area of the box of ref_nodes row i, f32, one rounding per
 * operation, no contraction, per component d = max - min:
 *     A(i) = 2.0f * ((dx * dy + dy * dz) + dz * dx)
 * A node is internal if and only if its left-child word (f32 3 of its row, as
 * int32) is >= 0. The growth of internal node i against a baseline `base` (the
 * areas of the same rows when the tree was built) is
 *     r(i) = A(i) / base[i]   if base[i] > 0   (correctly rounded f32 division)
 *          = 1.0f             otherwise.
 * The figure is the mean and the maximum of r over the internal nodes. Both are
 * exactly 1.0f on an unmoved or freshly built tree; the mean is scale-free and
 * grows monotonically as a refit tree's primitives scatter. Boxes are finite by
 * contract.
 *
 * ---- ptmi_tree_areas, in this order
 *
 * One lane per row i of ref_nodes, i in [0, num_bvh_nodes): areas[i] = A(i),
 * leaves included. With num_bvh_nodes == 0 nothing runs.
 *
 * ---- ptmi_tree_growth, in this order
 *
 * One launch of one workgroup of PTMI_TREE_GROWTH_LANES (1024) lanes.
 *   1. Lane k walks the rows k, k + 1024, k + 2048, ... below num_bvh_nodes in
 *      ascending order. It starts with an f64 sum of 0.0, an f32 maximum of
 *      1.0f and a count of 0. A leaf is skipped. For an internal node it adds
 *      (double)r(i) to its sum, takes max(m, r) = (m > r) ? m : r and counts 1.
 *   2. The lanes' values go to LDS, and for s = 512, 256, ..., 1, each step
 *      behind a barrier, lane k < s does
 *          sum[k] += sum[k + s]; max[k] = (max[k] > max[k + s]) ? max[k] : max[k + s];
 *          count[k] += count[k + s].
 *   3. Lane 0 writes out[0] = (float)(sum[0] / (double)n) with n = count[0], or
 *      1.0f with n == 0; out[1] = max[0]; out[2] = (float)n; out[3] = 0.0f.
 * The order of every addition is a function of num_bvh_nodes alone. With
 * num_bvh_nodes == 0 the launch still runs and writes {1, 1, 0, 0}.
 *
 * ---- ptmi_ids_remap, in this order
 *
 * One lane per element i in [0, n) of an id image (ptmi_motion.h: type << 28 |
 * device primitive index with type codes sphere 0, triangle 1, quad 2; -1 where
 * no surface shows). id = ids_in[i]; type = id >> 28, prim = id & 0x0fffffff.
 * The output is -1 if id < 0, if type > 2, if prim >= the type's count, or,
 * with m = map[prim] of the type's map (read only after the range check on
 * prim), if m is outside [0, count). Otherwise ids_out[i] = type << 28 | m.
 * ids_in == ids_out is allowed (each lane reads and writes its own element);
 * any other overlap of the two images is PTMI_EINVAL. With n == 0 nothing runs.
 *
 * ---- Call semantics
 *
 * Asynchronous on `stream`; no allocation; not timed by ptmi_prof_*. All
 * pointers but the scene view are device pointers, 4-byte aligned.
 */
#ifndef PTMI_TREE_H
#define PTMI_TREE_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_TREE_VERSION 1

/* The lanes of ptmi_tree_growth's one workgroup: part of the summation order. */
#define PTMI_TREE_GROWTH_LANES 1024

/* The primitive counts of the three id types, in type-code order. */
typedef struct ptmi_ids_counts {
    int32_t spheres;    /* type 0 */
    int32_t triangles;  /* type 1 */
    int32_t quads;      /* type 2 */
} ptmi_ids_counts;

/* areas[num_bvh_nodes] = the box areas of scene->ref_nodes. PTMI_EINVAL, each
 * with a message and before any HIP call: a NULL scene; a negative
 * num_bvh_nodes; NULL or misaligned ref_nodes or areas while num_bvh_nodes > 0. */
int ptmi_tree_areas(const ptmi_scene_view *scene, float *areas, void *stream);

/* out[4] = {mean, max, (float)n_inner_seen, 0} of scene->ref_nodes against
 * base_areas[num_bvh_nodes]. PTMI_EINVAL as for ptmi_tree_areas, base_areas in
 * the place of areas, and a NULL or misaligned out whatever the count (the call
 * always writes it). */
int ptmi_tree_growth(const ptmi_scene_view *scene, const float *base_areas, float *out, void *stream);

/* ids_out[n] = ids_in[n] with every primitive index sent through its type's
 * map (int32[count], old device row -> new device row). PTMI_EINVAL: a negative
 * n or count; a NULL or misaligned map of a type whose
 * count is > 0; NULL or misaligned ids_in or ids_out, or the two overlapping
 * without being equal, while n > 0. */
int ptmi_ids_remap(const int32_t *ids_in, int32_t *ids_out, int32_t n, const int32_t *map_spheres,
                   const int32_t *map_tris, const int32_t *map_quads, ptmi_ids_counts counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_TREE_H */
