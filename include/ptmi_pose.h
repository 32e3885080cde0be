/*
 * ptmi_pose.h — the pose ABI of libptmi.so: primitives of a resident scene that
 * move linearly over a shutter interval are put where they are at a time t, on
 * the device, from a resident track (a rest point and a displacement per
 * primitive), and the BVH above them is refitted. It is versioned apart from
 * PTMI_ABI_VERSION and from the versions of ptmi_post.h, ptmi_guide.h,
 * ptmi_temporal.h, ptmi_wf_tiles.h, ptmi_update.h, ptmi_motion.h, ptmi_tree.h,
 * ptmi_validate.h, ptmi_material.h and ptmi_build.h: nothing in them changes
 * with it, and no render kernel is involved. Error codes, ptmi_last_error(),
 * ptmi_scene_view and the row layouts are ptmi.h's; the topology, the refit and
 * the root copy are ptmi_update.h's.
 *
 * ---- Contract
 *
 * After the call the device holds, byte for byte, what ptmi_update_primitives
 * leaves when it is given the rows and builder-form records that the scene
 * compiler makes of the posed objects (ptmi/pose.py, posed_records(tracks, t)):
 *
 *   sphere    Sphere.stationary(o + t * d, radius, mat)
 *   quad      quad(Q + t * d, u, v, mat): normal, w, u and v are unchanged,
 *             D = normal . (Q + t * d)
 *   triangle  v0, v1, v2 each + t * d; edge1, edge2 and normal are those of the
 *             rest triangle (a pure translation keeps them to the last bit)
 *
 * ---- What one call does, in this order
 *
 * Step 1, pose_leaves, one lane per entry of every list. Entry i of a list of
 * type T names prim[i] and leaf[i] as an edit of ptmi_update_list does, and
 * rec[i], f64:
 *     sphere    6: {o.xyz, d.xyz}
 *     quad      9: {Q.xyz, d.xyz, normal.xyz}
 *     triangle 12: {v0.xyz, v1.xyz, v2.xyz, d.xyz}
 * Every component of a point is p + t * d in f64, the product rounded, then the
 * sum, no contraction, and is then cast to f32, round to nearest. The quad's D
 * is (n.x * Q'.x + n.y * Q'.y) + n.z * Q'.z in f64 on the uncast Q', then cast.
 * The lane writes only the row floats that change:
 *     sphere    f32 0 .. 2 (c); r stays
 *     quad      f32 3 (D) and 4 .. 6 (Q)
 *     triangle  f32 0 .. 2 (v0)
 * The builder-form record is formed from the new f32 points and the row's own r
 * (sphere), u and v (quad, f32 7 .. 12) or the cast v1' and v2' (triangle), and
 * the leaf box is computed from it by the rules of ptmi_update.h's step 1, pad
 * included, and written into min.xyz and max.xyz of ref_nodes[leaf[i]]. Inputs
 * are finite by contract and ids within one list distinct. An entry is skipped,
 * and touches nothing, exactly where an edit of ptmi_update_primitives is: prim
 * or leaf out of range, or a leaf code that does not name primitive prim[i] of
 * type T.
 *
 * Step 2 and the root copy are ptmi_update_primitives' own, in both forms
 * (topo->flags), by the same kernels.
 *
 * ---- Call semantics
 *
 * Asynchronous on `stream`; no allocation; not timed by ptmi_prof_*. Like an
 * update the call WRITES through the scene view's nodes, ref_nodes, spheres,
 * quads and tris: no render (or other reader) of this scene may be in flight
 * on another stream, and the view's host fields are the caller's to refresh. t = 0
 * is not the rest state byte for byte: Q + 0.0 * d turns a -0.0 into +0.0. The
 * rest state comes back by ptmi_update_primitives with the rest rows.
 */
#ifndef PTMI_POSE_H
#define PTMI_POSE_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"
#include "ptmi_update.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_POSE_VERSION 1

/* The tracks of one primitive type: device pointers, count entries each. */
typedef struct ptmi_pose_list {
    const int32_t *prim;   /* device primitive index */
    const int32_t *leaf;   /* ref_nodes index of its leaf */
    const double  *rec;    /* count x 6 / 9 / 12 f64, 8-B aligned:
                              sphere {o.xyz, d.xyz}; quad {Q.xyz, d.xyz, normal.xyz};
                              triangle {v0, v1, v2, d} */
    int32_t count;
} ptmi_pose_list;

/* Poses the tracked primitives at t and refits (see above). A NULL list is a
 * list of count 0; all counts zero is a pure refit. PTMI_EINVAL, each with a
 * message and before any HIP call: everything ptmi_update_primitives rejects
 * (with `rec`, 8-byte aligned, in place of `row` and `build`), and a t that is
 * not finite. */
int ptmi_pose_primitives(const ptmi_scene_view *scene, const ptmi_pose_list *spheres,
                         const ptmi_pose_list *quads, const ptmi_pose_list *tris, double t,
                         const ptmi_update_topology *topo, float *root_box, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_POSE_H */
