/*
 * ptmi_build.h — the device-build ABI of libptmi.so: the binned-SAH builder of
 * ptmi_bvh_build_sah (ptmi.h) run on the device, bit for bit, and the packer
 * that turns its arrays into the device layout of a resident scene, in the
 * tensors the scene already has. It is versioned apart from
 * the ten other headers (ptmi.h, ptmi_post.h, ptmi_guide.h, ptmi_temporal.h,
 * ptmi_wf_tiles.h, ptmi_update.h, ptmi_motion.h, ptmi_tree.h, ptmi_validate.h,
 * ptmi_material.h): nothing in them changes with it and no render kernel is
 * involved. Error codes, ptmi_last_error(), ptmi_scene_view and the layouts of
 * nodes, ref_nodes, the primitive rows and mats are ptmi.h's.
 *
 * ---- ptmi_build_sah_device
 *
 * Input: device arrays of builder-form records, as ptmi_bvh_build_sah takes
 * them on the host: spheres {c, r} (4 f32), quads {Q, u, v} (9 f32), triangles
 * {v0, v1, v2} (9 f32), finite by contract. The builder numbers the primitives
 * spheres, quads, triangles with type codes 0, 2, 1. Output: the seven
 * flattened arrays of 2 N - 1 nodes in preorder (bbox_min and bbox_max 3 f32
 * per node; left, right, parent, prim_type, prim_idx int32) and a status block
 * of PTMI_BUILD_STATUS_WORDS int32:
 *     [0] status: 0, or PTMI_BUILD_NEEDS_HOST
 *     [1] n_nodes (0 unless status is 0)
 *     [2] levels: iterations of the level loop
 *     [3] max_leaf_depth (root = 0)
 *     [4] nodes that took fallback entrance (a), [5] entrance (b)
 *     [6], [7] 0
 * With status 0 the arrays equal, bit for bit, what ptmi_bvh_build_sah writes
 * for the same records; with any other status they are unspecified. The device
 * never writes a different tree under status 0.
 *
 * One launch of one workgroup of PTMI_BUILD_LANES lanes walks the tree level by
 * level behind workgroup barriers: every open node of a level is a contiguous
 * segment of one id array, a subtree of k primitives has 2 k - 1 nodes, so a
 * node at index me whose left part has kL primitives has left = me + 1 and
 * right = me + 2 kL, and no traversal is needed. One workgroup is legitimate
 * because the call takes at most PTMI_BUILD_MAX_PRIMS primitives; a larger
 * scene is PTMI_ECAPACITY before any launch. Every box union and every
 * centroid minimum runs over its segment in id order, so a tie between -0.0
 * and +0.0 falls as on the host. The level loop ends when one LDS word (the
 * number of open segments), read by every lane after a barrier, is 0, and has
 * a hard bound of N iterations; each iteration shortens every open segment.
 *
 * The median fallback of the host builder has two entrances: (a) no split has
 * a finite cost (no axis with a centroid extent >= 1e-10, or a parent box
 * without area): the split position is the k/2-th order statistic of c[0]
 * under a stable sort; (b) the chosen position leaves one side empty: the
 * segment is stably sorted on the axis and cut at k/2. What the device handles
 * exactly: a segment of any length whose keys on the fallback axis are all
 * equal (the stable sort is the identity), and a segment of at most
 * PTMI_BUILD_SORT_MAX primitives with any keys (a stable rank count). A longer
 * segment with unequal keys writes status PTMI_BUILD_NEEDS_HOST.
 *
 * Zero primitives write the status block {0, 0, 0, 0, 0, 0, 0, 0} and nothing
 * else.
 *
 * ---- ptmi_build_pack
 *
 * What pack_device does after a rebuild, on the device, one launch of one
 * workgroup. It reads the builder's status block on the device and writes
 * nothing but info unless status is 0 and n_nodes is 2 N - 1 for the scene's N
 * primitives, so the host needs no synchronisation between the two calls.
 *   * slot of an internal node: the number of internal nodes before it in
 *     preorder; the new device row of a leaf's primitive: the number of leaves
 *     of its type before it in preorder (the leaf-order permutation).
 *   * primitive rows and the 80-byte mats rows are gathered from their old
 *     device rows into the new order, through the workspace. old_row[t]
 *     (int32[count]) maps a reference primitive index of type code t to its
 *     old device row.
 *   * a leaf's code is 0x80000000 | type << 28 | class << 25 | new row, the
 *     class that of the row's flags word (f32 19 of its mats row).
 *   * nodes rows: both child boxes interleaved per component (f32 0 - 11), the
 *     two child refs (12, 13; a leaf's code or an internal child's slot * 80),
 *     the children's centres (min + max) * 0.5f: z in 14, 15, x in 16, 17, y in
 *     18, 19. ref_nodes rows: {min, left | max, right | parent, code, side, 0}.
 *   * new_row[t] (int32[count]): old device row -> new device row; perm[t]
 *     (int32[count]): new device row -> reference primitive index.
 *   * info, PTMI_BUILD_INFO_WORDS 4-byte words: [0] root_ref, [1]
 *     max_leaf_depth, [2] internal nodes, [3] nodes, [4 - 6] the root box's
 *     minimum and [7 - 9] its maximum (f32), [10] the pack's own status: 0
 *     packed, PTMI_BUILD_PACK_SKIPPED (the builder's status was not 0 or its
 *     node count another), PTMI_BUILD_PACK_REJECTED (the arrays are no preorder
 *     tree of the scene's primitives; nothing else was written), [11] 0.
 * It writes through the view's pointers, so no render of the scene may be in
 * flight (ptmi_update.h's rule).
 *
 * ---- Call semantics
 *
 * Asynchronous on `stream`; no allocation; not timed by ptmi_prof_*. All
 * pointers but the scene view and the structs that carry them are device
 * pointers. The records, the seven built arrays, status, info, the maps and
 * the view's ref_nodes are 4-byte aligned; the view's nodes, mats and the row
 * arrays of its three primitive types, and the workspace, are 16-byte aligned
 * (ptmi.h's rows). The workspace belongs to the call until the stream has
 * passed it. Every rejected argument is
 * PTMI_EINVAL with a message before any HIP call.
 */
#ifndef PTMI_BUILD_H
#define PTMI_BUILD_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_BUILD_VERSION 1

/* The most primitives the one-workgroup builder and packer take. */
#define PTMI_BUILD_MAX_PRIMS 4096
/* The lanes of their one workgroup. */
#define PTMI_BUILD_LANES 1024
/* The longest fallback segment with unequal keys the device sorts itself. */
#define PTMI_BUILD_SORT_MAX 1024

#define PTMI_BUILD_STATUS_WORDS 8
#define PTMI_BUILD_INFO_WORDS 12
#define PTMI_BUILD_NEEDS_HOST 1
#define PTMI_BUILD_PACK_SKIPPED 1
#define PTMI_BUILD_PACK_REJECTED 2

/* The seven flattened arrays, on the device: room for 2 N - 1 nodes each. */
typedef struct ptmi_build_arrays {
    float *bbox_min;   /* 3 f32 per node */
    float *bbox_max;
    int32_t *left;
    int32_t *right;
    int32_t *parent;
    int32_t *prim_type;
    int32_t *prim_idx;
} ptmi_build_arrays;

/* One int32 device array per primitive type, in type-code order; an array of a type without primitives may be NULL. */
typedef struct ptmi_build_maps {
    int32_t *spheres;    /* type 0 */
    int32_t *triangles;  /* type 1 */
    int32_t *quads;      /* type 2 */
} ptmi_build_maps;

/* Bytes of the workspace both calls below need for n_prims primitives: 0 for a count they do not take (negative, or
 * above PTMI_BUILD_MAX_PRIMS), non-decreasing otherwise. */
size_t ptmi_build_workspace_bytes(int32_t n_prims);

/* PTMI_EINVAL: a negative count; NULL or misaligned records of a type whose count is > 0; a NULL or misaligned status;
 * with N > 0 a NULL or misaligned output array or workspace (16 bytes), or workspace_bytes below
 * ptmi_build_workspace_bytes(N). PTMI_ECAPACITY: N > PTMI_BUILD_MAX_PRIMS. */
int ptmi_build_sah_device(const float *spheres, int32_t ns, const float *quads, int32_t nq, const float *tris,
                          int32_t nt, const ptmi_build_arrays *out, int32_t *status, void *workspace,
                          size_t workspace_bytes, void *stream);

/* PTMI_EINVAL: a NULL scene, arrays, old_row, new_row or perm; negative counts; a NULL or misaligned status or info;
 * with N > 0 a view whose num_bvh_nodes is not 2 N - 1 or whose n_inner is not N - 1; a NULL or misaligned scene
 * array that the call writes (nodes with N > 1, mats and the rows of a type with primitives: 16 bytes; ref_nodes:
 * 4 bytes), built array, map of a type with primitives, or workspace (16 bytes); workspace_bytes below
 * ptmi_build_workspace_bytes(N). PTMI_ECAPACITY: N > PTMI_BUILD_MAX_PRIMS. With N == 0 nothing runs. */
int ptmi_build_pack(const ptmi_scene_view *scene, const ptmi_build_arrays *built, const int32_t *status,
                    const ptmi_build_maps *old_row, const ptmi_build_maps *new_row, const ptmi_build_maps *perm,
                    int32_t *info, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_BUILD_H */
