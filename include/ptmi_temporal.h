/*
 * ptmi_temporal.h — the temporal ABI of libptmi.so: reprojection of a stats
 * render's history (accum and stats, ptmi.h) from the previous camera to the
 * current one, by the first-hit guide images of both (ptmi_guide.h). It is
 * versioned apart from PTMI_ABI_VERSION, PTMI_POST_VERSION and
 * PTMI_GUIDE_VERSION: nothing in ptmi.h, ptmi_post.h or ptmi_guide.h changes
 * with it. Error codes, ptmi_last_error() and ptmi_camera are ptmi.h's; the
 * guide image {nx, ny, nz, depth, ar, ag, ab, hit} is ptmi_guide.h's.
 *
 * All arithmetic is f32 with one rounding per operation (-ffp-contract=off,
 * correctly rounded / and sqrtf), in the order written here.
 *   dot(x, x') = (x*x' + y*y') + z*z';
 *   cross(a, b)_x = a_y*b_z - a_z*b_y (two products, one subtraction), cyclic;
 *   lum(c) = (0.2126f*r + 0.7152f*g) + 0.0722f*b (ptmi_post.h's);
 *   every comparison is false for NaN.
 * Whole frames on one device, like the guides. The scene is static: a surface
 * point is where it was.
 *
 * ---- ptmi_reproject
 *
 * Per pixel (px, py) of the current frame, g = guides_cur[py][px]:
 *
 * 1. ps = (cur.pixel00 + cur.delta_u * (float)px) + cur.delta_v * (float)py;
 *    d = ps - cur.center; len = sqrtf(dot(d, d)): as ptmi_guide_trace forms
 *    them.
 * 2. g.hit != 0: s = g.depth / len, P_k = cur.center_k + d_k * s,
 *    v = P - prev.center. Otherwise (a miss, a point at infinity): v = d.
 * 3. r = prev.pixel00 - prev.center; w = cross(prev.delta_u, prev.delta_v);
 *    lam = dot(r, w) / dot(v, w); q_k = v_k * lam - r_k;
 *    a = dot(q, prev.delta_u) / dot(prev.delta_u, prev.delta_u);
 *    b = dot(q, prev.delta_v) / dot(prev.delta_v, prev.delta_v);
 *    zexp = sqrtf(dot(v, v)).
 *    (a, b) is the previous frame's pixel position of the point. This takes
 *    prev.delta_u perpendicular to prev.delta_v, which every camera ptmi
 *    uploads satisfies; for another camera the position is wrong, not unsafe.
 * 4. The pixel is geometrically valid iff
 *      lam > 0 && a > -1 && a < (float)width && b > -1 && b < (float)height.
 *    Only then x0 = floorf(a), fx = a - x0, y0 = floorf(b), fy = b - y0 and
 *    the conversion of x0, y0 to int happen.
 * 5. Four taps q = (x0 + i, y0 + j), j outer and i inner, both ascending, of
 *    weight wt = (i ? fx : 1 - fx) * (j ? fy : 1 - fy). A tap counts iff all of
 *      - it lies inside the image;
 *      - n_q = stats_prev[q][0] >= 2;
 *      - c_q = accum_prev[q] * (float)(1.0 / (double)n_q) per channel and
 *        s2_q = stats_prev[q][2] / (n_q - 1) are finite;
 *      - (hit_q != 0) == (hit_p != 0), the guides of q from guides_prev and of
 *        p from guides_cur;
 *      - for hits: fabsf(z_q - zexp) <= sigma_z * zexp + 1e-4f,
 *        dot(n_p, n_q) >= normal_min, and
 *        (|ar_p - ar_q| + |ag_p - ag_q|) + |ab_p - ab_q| <= sigma_a.
 * 6. Sequential sums over the counted taps: W += wt, C += wt * c_q per channel,
 *    S += wt * s2_q, N += wt * n_q.
 * 7. If the pixel is valid and W > 0: c' = C / W, s2' = S / W,
 *    n' = floorf(fminf(N / W, max_history)), and if n' >= 1
 *      accum_out = c' * n', stats_out = {n', lum(c'), s2' * (n' - 1), 0}.
 *    In every other case both are written as zeros: the state ptmi_clear and
 *    the stats clear leave, a pixel without history.
 *
 * So the carried variance is the plain weighted mean of the taps' per-sample
 * variances (interpolated taps are correlated: the reprojection claims no noise
 * reduction), n' is integer-valued, and a NaN pixel of the history is skipped
 * as a tap and does not spread.
 */
#ifndef PTMI_TEMPORAL_H
#define PTMI_TEMPORAL_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_TEMPORAL_VERSION 1

typedef struct ptmi_reproject_params {
    float max_history; /* cap on the carried sample count, 1 .. 16777216 */
    float sigma_z;     /* relative depth tolerance, >= 0 */
    float normal_min;  /* least normal dot product, -1 .. 1 */
    float sigma_a;     /* largest L1 albedo distance, >= 0 */
    int32_t flags;     /* must be 0 */
} ptmi_reproject_params;

/* The reprojection above: one kernel, one lane per current pixel.
 * guides_cur, guides_prev: [height][width][8]; accum_prev, accum_out:
 * [height][width][3]; stats_prev, stats_out: [height][width][4]. Asynchronous
 * on `stream`, graph-capturable, no allocation, not timed by ptmi_prof_*.
 * PTMI_EINVAL, each with a message and before any HIP call: a NULL pointer;
 * width or height < 1 (or more than 2^31-1 pixels); guides or stats pointers
 * not 16-byte aligned; an output overlapping any input or the other output;
 * max_history NaN, < 1 or > 2^24; sigma_z or sigma_a negative or NaN;
 * normal_min NaN or outside [-1, 1]; flags != 0. */
int ptmi_reproject(const ptmi_camera *cur, const ptmi_camera *prev, const float *guides_cur,
                   const float *guides_prev, const float *accum_prev, const float *stats_prev, int32_t width,
                   int32_t height, const ptmi_reproject_params *params, float *accum_out, float *stats_out,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_TEMPORAL_H */
