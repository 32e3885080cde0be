/*
 * ptmi_motion.h — the motion ABI of libptmi.so: temporal reprojection
 * (ptmi_temporal.h) across a scene update (ptmi_update.h). The guide trace also
 * writes which primitive each pixel sees, and the reprojection finds, for a
 * pixel of the new frame, where its surface point was on that primitive before
 * the update. It is versioned apart from PTMI_ABI_VERSION and the versions of
 * the other five headers: nothing in ptmi.h, ptmi_post.h, ptmi_guide.h,
 * ptmi_temporal.h, ptmi_wf_tiles.h or ptmi_update.h changes with it. Error
 * codes, ptmi_last_error(), ptmi_scene_view, ptmi_frame and ptmi_camera are
 * ptmi.h's; the guide image is ptmi_guide.h's; ptmi_reproject_params and the
 * steps 1 - 7 referred to below are ptmi_temporal.h's.
 *
 * All arithmetic is f32 with one rounding per operation (-ffp-contract=off,
 * correctly rounded / and sqrtf), in the order written here; dot and cross are
 * ptmi_temporal.h's:
 *   dot(x, x') = (x*x' + y*y') + z*z';
 *   cross(a, b)_x = a_y*b_z - a_z*b_y (two products, one subtraction), cyclic;
 *   a vector times a scalar, and a sum of vectors, per component;
 *   every comparison is false for NaN.
 * Whole frames on one device, like the guides.
 *
 * ---- The id image (ptmi_guide_trace_ids)
 *
 * ids[height][width] int32. A pixel whose guide pixel is a surface hit holds
 *   type << 28 | prim
 * the leaf code (ptmi.h) of the surface the guide pixel describes, with bit 31
 * and the class bits cleared: type 0 sphere, 1 triangle, 2 quad; prim the
 * device primitive index, the row of the scene view's spheres, tris or quads.
 * Every other pixel holds -1: a miss, and a medium hit in the fourth traversal.
 * guides is byte for byte what ptmi_guide_trace writes.
 *
 * ---- ptmi_reproject_moved
 *
 * The rows of the scene view are the current ones (after the update), the
 * prev_* arrays hold the same rows as they were before it. Per pixel p =
 * (px, py) of the current frame, ptmi_reproject's steps 1 - 7 with two changes.
 *
 * 2'. g.hit == 0 (a miss): v = d, as in step 2. Otherwise P_k = cur.center_k +
 *     d_k * s with s = g.depth / len as in step 2, id = ids_cur[p], and
 *       - id < 0, or type = id >> 28 not 0, 1 or 2, or prim = id & 0x0fffffff
 *         not below the count of its type: the pixel has no history. Zeros are
 *         written and nothing is read through the id.
 *       - the primitive's current row and its previous row are bitwise equal:
 *         P_prev = P, with no arithmetic. An unmoved primitive reproduces
 *         ptmi_reproject bit for bit.
 *       - sphere, row {c, r}: k = r_old / r_new;
 *         P_prev = c_old + (P - c_new) * k.
 *       - quad, row {n, D, Q, u, v, w}: h = P - Q_new;
 *         alpha = dot(w_new, cross(h, v_new)); beta = dot(w_new, cross(u_new, h));
 *         P_prev = (Q_old + u_old * alpha) + v_old * beta.
 *       - triangle, row {v0, e1, e2, n}: h = P - v0_new;
 *         m = cross(e1_new, e2_new); mm = dot(m, m);
 *         alpha = dot(cross(h, e2_new), m) / mm;
 *         beta = dot(cross(e1_new, h), m) / mm;
 *         P_prev = (v0_old + e1_old * alpha) + e2_old * beta.
 *     Then v = P_prev - prev.center, and steps 3 - 7 follow as written. A
 *     non-finite P_prev makes step 4's comparisons false: no history.
 * 5'. With PTMI_RPM_MATCH_IDS a tap q of a hit pixel also needs
 *     ids_prev[q] == ids_cur[p]. The depth, normal and albedo tests stay. The
 *     taps of a miss pixel are step 5's.
 *
 * So the point keeps its place on the primitive: its direction and relative
 * distance from a sphere's centre, its (alpha, beta) on a quad, its barycentric
 * coordinates on a triangle. Two consequences:
 *   - A surface whose normal turned by more than normal_min allows loses its
 *     history: step 5 compares the normal of the current frame with the one
 *     the previous frame recorded. The same holds for a depth that changed by
 *     more than sigma_z allows between P_prev's distance and the recorded one.
 *   - Lighting that changed because of the move (the moved object's shadow,
 *     its reflection in another surface) is not detected: those pixels see
 *     primitives that did not move and keep their history. max_history bounds
 *     how long it lags, as for any temporal filter.
 * Media have no id: a pixel seen through a medium boundary that moved is
 * treated by the surface behind it.
 */
#ifndef PTMI_MOTION_H
#define PTMI_MOTION_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"
#include "ptmi_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_MOTION_VERSION 1

#define PTMI_RPM_MATCH_IDS 1 /* ptmi_reproject_moved_params.flags, bit 0 */

/* The guide trace of ptmi_guide.h that also writes the id image above: the
 * same kernel with one more dword store per pixel. Asynchronous on `stream`,
 * graph-capturable, no allocation, not timed by ptmi_prof_*. PTMI_EINVAL, each
 * with a message and before any HIP call: whatever ptmi_guide_trace rejects; a
 * NULL ids or one not 4-byte aligned; ids overlapping guides or an array of
 * the scene view. */
int ptmi_guide_trace_ids(const ptmi_scene_view *scene, const ptmi_frame *frame, float *guides, int32_t *ids,
                         void *stream);

typedef struct ptmi_reproject_moved_params {
    ptmi_reproject_params base; /* as for ptmi_reproject; base.flags must be 0 */
    int32_t flags;              /* bit 0: PTMI_RPM_MATCH_IDS; other bits must be 0 */
} ptmi_reproject_moved_params;

/* The reprojection above: one kernel, one lane per current pixel. The images
 * are ptmi_reproject's; ids_cur, ids_prev: [height][width] int32. Of `scene`
 * only spheres, quads, tris and their three counts are read (the current
 * rows); prev_spheres, prev_quads, prev_tris: device arrays of the same layout
 * and counts, the rows before the update; one may be NULL when its count is 0.
 * Asynchronous on `stream`, graph-capturable, no allocation, not timed by
 * ptmi_prof_*. PTMI_EINVAL, each with a message and before any HIP call:
 * everything ptmi_reproject rejects; a NULL scene or params; an id image NULL
 * or not 4-byte aligned; a count below 0 or above 2^25; a row array of a count
 * above 0 that is NULL or not 16-byte aligned; an output overlapping any
 * input, the id images and the six row arrays included, or the other output;
 * unknown flag bits. */
int ptmi_reproject_moved(const ptmi_camera *cur, const ptmi_camera *prev, const float *guides_cur,
                         const float *guides_prev, const float *accum_prev, const float *stats_prev,
                         const int32_t *ids_cur, const int32_t *ids_prev, const ptmi_scene_view *scene,
                         const float *prev_spheres, const float *prev_quads, const float *prev_tris, int32_t width,
                         int32_t height, const ptmi_reproject_moved_params *params, float *accum_out,
                         float *stats_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_MOTION_H */
