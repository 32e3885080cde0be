/*
 * ptmi_rigid.h — the rigid-body pose ABI of libptmi.so: groups of primitives of
 * a resident scene (bodies) that turn about an axis and move over a shutter
 * interval are put where they are at a time t, on the device, from resident
 * rest records in f64 and a small table of body transforms the host evaluates,
 * and the BVH above them is refitted. It is versioned apart from
 * PTMI_ABI_VERSION and from the versions of ptmi_post.h, ptmi_guide.h,
 * ptmi_temporal.h, ptmi_wf_tiles.h, ptmi_update.h, ptmi_motion.h, ptmi_tree.h,
 * ptmi_validate.h, ptmi_material.h, ptmi_build.h and ptmi_pose.h: nothing in
 * them changes with it, and no render kernel is involved. Error codes,
 * ptmi_last_error(), ptmi_scene_view and the row layouts are ptmi.h's; the
 * topology, the refit and the root copy are ptmi_update.h's.
 *
 * ---- Contract
 *
 * After the call the device holds, byte for byte, what ptmi_update_primitives
 * leaves when it is given the rows and builder-form records that the scene
 * compiler makes of the posed objects (ptmi/rigid.py, posed_records(bodies,
 * prims, t)).
 *
 * A body at time t is 15 doubles: R, the rotation by turn * t about its axis
 * (row-major, Rodrigues' formula evaluated on the host: the device never
 * evaluates a sine), its pivot c and the moved pivot c'(t) = c + t * d. With
 * every product rounded, then the sums in this order, no contraction:
 *
 *   a point   q = p - c;  r[k] = (R[k][0]*q.x + R[k][1]*q.y) + R[k][2]*q.z;  p' = r + c'
 *   a vector  v'[k] = (R[k][0]*v.x + R[k][1]*v.y) + R[k][2]*v.z
 *
 *   sphere    Sphere.stationary(p'(center), radius, mat)
 *   quad      Q' = p'(Q); u, v, normal and w are each R * the REST quad's f64
 *             vector; D' = (n'.x*Q'.x + n'.y*Q'.y) + n'.z*Q'.z on the uncast values
 *   triangle  v0', v1', v2' = p'(...); edge1, edge2 and normal are each R * the
 *             rest triangle's
 *
 * The rest object's own unit normal, w and edges are rotated, not formed anew
 * from the posed points: that needs only f64 add, subtract and multiply. A
 * posed normal is therefore a unit vector only to f64 rounding. With R the
 * identity and c' = c every row float compares == to the rest row (a -0.0 may
 * become +0.0).
 *
 * ---- What one call does, in this order
 *
 * Step 1, rigid_leaves, one lane per entry of every list. Entry i of a list of
 * type T names prim[i] and leaf[i] as an edit of ptmi_update_list does, its
 * body body[i] (an index into `bodies`), and its rest record rec[i], f64:
 *     sphere    3: {c.xyz}
 *     quad     15: {Q.xyz, u.xyz, v.xyz, normal.xyz, w.xyz}
 *     triangle 18: {v0.xyz, v1.xyz, v2.xyz, e1.xyz, e2.xyz, n.xyz}
 * Every value is computed in f64 as above and then cast to f32, round to
 * nearest. The lane writes
 *     sphere    f32 0 .. 2 (c); r stays
 *     quad      the whole row {normal, D, Q, u, v, w}
 *     triangle  the whole row {v0, e1, e2, n}
 * forms the builder-form record from the new f32 values (sphere c', r; quad Q',
 * u', v'; triangle the cast v0', v1', v2'), computes the leaf box from it by the
 * rules of ptmi_update.h's step 1, pad included, and writes it into min.xyz and
 * max.xyz of ref_nodes[leaf[i]]. Inputs are finite by contract and ids within
 * one list distinct. An entry is skipped, and touches nothing, exactly where an
 * edit of ptmi_update_primitives is (prim or leaf out of range, or a leaf code
 * that does not name primitive prim[i] of type T), and also where body[i] is
 * outside [0, n_bodies).
 *
 * Step 2 and the root copy are ptmi_update_primitives' own, in both forms
 * (topo->flags), by the same kernels.
 *
 * ---- Call semantics
 *
 * Asynchronous on `stream`; no allocation; not timed by ptmi_prof_*. `bodies`
 * is HOST memory: it is read before the call returns and passed to the kernel
 * by value (PTMI_RIGID_MAX_BODIES x 120 B = 1920 B of kernel arguments), so
 * there is no upload, no buffer to keep alive and nothing to race with. Like an
 * update the call WRITES through the scene view's nodes, ref_nodes, spheres,
 * quads and tris: no render (or other reader) of this scene may be in flight on
 * another stream, and the view's host fields are the caller's to refresh. The
 * rest state comes back by ptmi_update_primitives with the rest rows.
 */
#ifndef PTMI_RIGID_H
#define PTMI_RIGID_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"
#include "ptmi_update.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_RIGID_VERSION 1
#define PTMI_RIGID_MAX_BODIES 16

/* One body at one time: row-major R; the pivot c; the moved pivot c'(t). */
typedef struct ptmi_rigid_body {
    double R[9];
    double pivot[3];
    double pivot_t[3];
} ptmi_rigid_body;

/* The entries of one primitive type: device pointers, count entries each. */
typedef struct ptmi_rigid_list {
    const int32_t *prim;   /* device primitive index */
    const int32_t *leaf;   /* ref_nodes index of its leaf */
    const int32_t *body;   /* index into `bodies` */
    const double  *rec;    /* count x 3 / 15 / 18 f64, 8-B aligned (see above) */
    int32_t count;
} ptmi_rigid_list;

/* Poses the bodies' primitives and refits (see above). A NULL list is a list of
 * count 0; all counts zero is a pure refit. PTMI_EINVAL, each with a message
 * and before any HIP call: everything ptmi_pose_primitives rejects but its t
 * (with `rec`, 8-byte aligned); `body` NULL or not 4-byte aligned where count >
 * 0; n_bodies outside [0, PTMI_RIGID_MAX_BODIES]; `bodies` NULL with n_bodies >
 * 0; any of the 15 doubles of one of the n_bodies bodies not finite. */
int ptmi_pose_rigid(const ptmi_scene_view *scene, const ptmi_rigid_list *spheres,
                    const ptmi_rigid_list *quads, const ptmi_rigid_list *tris,
                    const ptmi_rigid_body *bodies /* HOST memory */, int32_t n_bodies,
                    const ptmi_update_topology *topo, float *root_box, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_RIGID_H */
