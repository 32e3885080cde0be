/*
 * ptmi_material.h — the material-edit ABI of libptmi.so: material rows of a
 * resident scene are replaced in place on the device, and the leaf codes that
 * carry each primitive's material class are patched with them. It is versioned
 * apart from PTMI_ABI_VERSION, PTMI_POST_VERSION, PTMI_GUIDE_VERSION,
 * PTMI_TEMPORAL_VERSION, PTMI_WF_TILES_VERSION, PTMI_UPDATE_VERSION,
 * PTMI_MOTION_VERSION, PTMI_TREE_VERSION and PTMI_VALIDATE_VERSION: nothing in
 * the other headers changes with it, and no render kernel is involved. Error
 * codes, ptmi_last_error(), ptmi_scene_view, PTMI_CLASS_* and the layouts of
 * mats, nodes and ref_nodes are ptmi.h's.
 *
 * ---- Why a row cannot simply be copied
 *
 * ptmi.h packs the material class of a primitive into its leaf code,
 *     0x80000000 | type << 28 | class << 25 | primitive index,
 * and the code is stored twice: in word 9 of the leaf's ref_nodes row (the
 * stackless traversal) and as child ref f32 12 or 13 of the parent's nodes row
 * (the stack traversal). The wavefront sorts hits by that class without
 * loading the material, and the shell hint claims that its sphere has class
 * PTMI_CLASS_MEDIUM. A mats row whose flags name another class than its leaf
 * codes do is therefore an invalid scene. This call keeps the three in step.
 *
 * ---- What one call does
 *
 * One kernel, mat_edit, one lane per edit of every list. Edit i of a list of
 * type T (sphere, quad, triangle) names
 *     prim[i]   the device primitive index (device order is leaf order),
 *     leaf[i]   the ref_nodes index of that primitive's leaf,
 *     row[i]    its new mats row: 20 f32 as ptmi.h lays them out, the last
 *               one the flags word (u32 bits)
 *               mat_type | tex_type << 4 | is_medium << 8 | (image index + 1) << 16.
 *
 * 1. The edit is skipped, and touches nothing, if prim[i] is outside [0, the
 *    type's primitive count), if leaf[i] is outside [0, num_bvh_nodes), if the
 *    leaf code stored in word 9 of ref_nodes[leaf[i]] does not name primitive
 *    prim[i] of type T, or if the new flags' image index + 1 (bits 16 - 31)
 *    exceeds scene->num_images (the row would read texels that are not there).
 * 2. row[i] is copied over row base_T + prim[i] of mats. The blocks of mats
 *    lie in storage order, spheres, quads, triangles: base = 0, num_spheres,
 *    num_spheres + num_quads. (The type codes of a leaf code are another
 *    order: sphere 0, triangle 1, quad 2.)
 * 3. class = mat_class(flags), from the new flags word alone: is_medium gives
 *    PTMI_CLASS_MEDIUM; else tex_type 3 (Perlin noise) on mat_type 0
 *    (Lambertian) or 4 (isotropic) gives PTMI_CLASS_NOISE; else mat_type 0
 *    gives PTMI_CLASS_LAMBERTIAN, 2 PTMI_CLASS_DIELECTRIC, 3
 *    PTMI_CLASS_EMISSIVE and anything else PTMI_CLASS_GLOSSY.
 * 4. The class bits (25 - 27) of the leaf code are replaced and nothing else
 *    in it changes. The new code is stored to word 9 of ref_nodes[leaf[i]],
 *    and, with parent = word 8 and side = word 10 of that row, to f32
 *    12 + side of row slot[parent] of nodes. A leaf that is the root
 *    (parent < 0) has no nodes store: its code is the view's root_ref, a host
 *    field that the caller refreshes. A parent outside [0, num_bvh_nodes), a
 *    side other than 0 or 1 or a slot outside [0, n_inner) skips the nodes
 *    store only.
 *
 * Ids within one list must be distinct. A row equal to the one the primitive
 * has changes no byte, and an edit followed by its inverse restores every byte.
 *
 * ---- Call semantics
 *
 * Asynchronous on `stream`; no allocation; not timed by ptmi_prof_*. The call
 * WRITES through the scene view's mats, nodes and ref_nodes pointers, although
 * the view declares them const: the caller must have no render (or any other
 * reader) of this scene in flight on another stream, and orders later renders
 * after the call as after any work on `stream`. The view's host fields
 * (root_ref, shell) are the caller's to refresh: root_ref where the root is a
 * leaf; the shell hint is a claim about a sphere's class (ptmi.h) that an edit
 * can break or establish, and 0 is always valid.
 */
#ifndef PTMI_MATERIAL_H
#define PTMI_MATERIAL_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_MATERIAL_VERSION 1

/* The edits of one primitive type: device pointers, count entries each. */
typedef struct ptmi_material_list {
    const int32_t *prim;   /* device primitive index (row of spheres / quads / tris) */
    const int32_t *leaf;   /* ref_nodes index of that primitive's leaf */
    const float *row;      /* count x 20 f32, a mats row as ptmi.h lays it out */
    int32_t count;
} ptmi_material_list;

/* Applies the edits (see above). A NULL list is a list of count 0; all counts
 * zero is a no-op that returns 0. `slot` is ptmi_update_topology's: device
 * int32[num_bvh_nodes], the row in nodes of each internal node, -1 for leaves.
 * PTMI_EINVAL, each with a message and before any HIP call: a NULL scene; a
 * negative count or one above the type's primitive count; a NULL or misaligned
 * (4 B) pointer of a list with count > 0; NULL mats or ref_nodes with any
 * count > 0; NULL nodes or slot with n_inner > 0 and any count > 0. */
int ptmi_update_materials(const ptmi_scene_view *scene, const ptmi_material_list *spheres,
                          const ptmi_material_list *quads, const ptmi_material_list *tris,
                          const int32_t *slot, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_MATERIAL_H */
