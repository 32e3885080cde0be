/*
 * ptmi_validate.h — the history-validation ABI of libptmi.so: a carried history
 * (ptmi_reproject's or ptmi_reproject_moved's output) is compared with a few
 * fresh samples of the current scene, pooled over a window, and the part of it
 * whose radiance no longer agrees is dropped before the two are merged. The
 * reprojections accept a tap when the surface is the same; this call asks
 * whether the light on it still is. It is versioned apart from
 * PTMI_ABI_VERSION, PTMI_POST_VERSION, PTMI_GUIDE_VERSION,
 * PTMI_TEMPORAL_VERSION, PTMI_WF_TILES_VERSION, PTMI_UPDATE_VERSION,
 * PTMI_MOTION_VERSION and PTMI_TREE_VERSION: nothing in ptmi.h, ptmi_post.h,
 * ptmi_guide.h, ptmi_temporal.h, ptmi_wf_tiles.h, ptmi_update.h, ptmi_motion.h
 * or ptmi_tree.h changes with it, and no render kernel is involved. Error
 * codes and ptmi_last_error() are ptmi.h's; the layouts of an accumulator
 * (H x W x 3 f32, a sum of sample colours) and of a stats image (H x W x 4 f32,
 * {n, mean, M2, 0} of the sample luminance, 16-byte aligned) are ptmi.h's too.
 *
 * ---- The arithmetic, in this order
 *
 * Everything is f32 with one rounding per operation, in the order written, no
 * contraction, correctly rounded / and sqrtf. Subscript h is the history pixel,
 * f the fresh pixel; finite(x) is "neither NaN nor an infinity".
 *
 * 1. Per pixel q, from the two stats pixels alone. q is usable if and only if
 *    n_h >= 2, n_f >= 2 and n_h, mean_h, M2_h, n_f, mean_f, M2_f are all
 *    finite. For a usable q
 *        d_q = mean_f - mean_h
 *        v_q = (M2_h / (n_h - 1)) / n_h + (M2_f / (n_f - 1)) / n_f
 *    (the difference of the two means and the variance of that difference);
 *    otherwise d_q = v_q = 0.
 *
 * 2. The window of pixel p = (x, y) is the pixels (x + i, y + j) with i, j in
 *    [-radius, radius] that lie inside the image. With j outer and i inner,
 *    both ascending, and D = V = 0.0f, m = 0 at the start:
 *        D = D + d_q;  V = V + v_q;  m = m + 1 if q is usable.
 *    (An unusable pixel adds 0.0f, which changes no bit of a sum that began at
 *    +0.0f; adding it or skipping it is the same.)
 *
 * 3. The stale fraction lam of p, the first case that holds:
 *        m == 0                      lam = 0   (nothing to judge by)
 *        D or V is NaN               lam = 1
 *        V > 0                       z = fabsf(D) / sqrtf(V);
 *                                    lam = 1 if z is NaN (inf / inf), else
 *                                    lam = fminf(fmaxf((z - k_lo) / (k_hi - k_lo), 0.0f), 1.0f)
 *        V == 0                      lam = (D == 0) ? 0 : 1
 *        otherwise (V < 0)           lam = 1   (a negative M2 is no variance)
 *
 * 4. The history pixel of p is empty if any of its three accum values or its
 *    n, mean or M2 is not finite: then n_h = 0 and mean_h = M2_h = 0 and its
 *    accum counts as 0 from here on (step 1 has already run and read only the
 *    stats). The validated count, integer-valued for an integer n_h:
 *        n_v = floorf(n_h * (1.0f - lam))
 *
 * 5. The merge.
 *        c_h  = hist_accum * (float)(1.0 / (double)fmaxf(n_h, 1.0f))    per channel
 *        A_v  = c_h * n_v                                              per channel
 *        M2_v = (n_h >= 2 && n_v >= 1) ? (M2_h / (n_h - 1.0f)) * (n_v - 1.0f) : 0
 *    except that with n_v == n_h (nothing is dropped) the history is taken as
 *    it is: A_v = hist_accum and M2_v = M2_h, bit for bit. (c_h * n_h need not
 *    round back to hist_accum, nor (M2_h / (n_h - 1)) * (n_h - 1) to M2_h; a
 *    history that passes must pass unchanged.)
 *        n_v < 1     the output pixel is the fresh pixel, all seven words.
 *        n_f == 0    out_accum = A_v, out_stats = {n_v, mean_h, M2_v, 0}.
 *        otherwise   delta = mean_f - mean_h;  n = n_v + n_f
 *                    out_accum = A_v + fresh_accum                     per channel
 *                    mean = mean_h + delta * (n_f / n)
 *                    M2   = (M2_v + M2_f) + (delta * delta) * ((n_v * n_f) / n)
 *                    out_stats = {n, mean, M2, 0}
 *    The cases are tested in this order. A NaN fresh pixel therefore passes
 *    through to its own output pixel, as it does in a uniform render, and to no
 *    other: step 1 leaves it out of every window.
 *
 * 6. weight_out[p], if asked for: (n_h >= 1) ? n_v / n_h : 0, with step 4's n_h.
 *
 * An empty history gives the fresh pair back byte for byte, an empty fresh pair
 * the history (m is 0 everywhere, so lam is 0 and n_v == n_h).
 *
 * ---- Call semantics
 *
 * Asynchronous on `stream`, graph-capturable (one kernel node), no allocation,
 * whole frames on one device, not timed by ptmi_prof_*. All image pointers are
 * device pointers. Not in place: out_accum, out_stats and weight_out must not
 * overlap any input or each other.
 */
#ifndef PTMI_VALIDATE_H
#define PTMI_VALIDATE_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_VALIDATE_VERSION 1

/* The largest window radius: a 16 x 16 tile and its halo are at most 30 x 30 pixels. */
#define PTMI_VALIDATE_MAX_RADIUS 7

typedef struct ptmi_validate_params {
    int32_t radius; /* the window is (2 * radius + 1)^2 pixels; 0 .. 7, default 3 */
    float k_lo;     /* |D| / sqrt(V) up to which all history is kept; >= 0, default 2 */
    float k_hi;     /* ... and from which none is; > k_lo, default 4 */
} ptmi_validate_params;

/* out = hist validated against fresh and merged with it. PTMI_EINVAL, each with
 * a message and before any HIP call: a NULL hist_accum, fresh_accum or
 * out_accum, or one not 4-byte aligned; a NULL hist_stats, fresh_stats or
 * out_stats, or one not 16-byte aligned; a NULL params; a weight_out that is
 * not NULL and not 4-byte aligned; width or height < 1 or more than 2^31-1
 * pixels; radius outside 0 .. 7; a k_lo or k_hi that is not finite; k_lo < 0;
 * k_hi not above k_lo; out_accum, out_stats or weight_out overlapping an input
 * or one another. */
int ptmi_history_validate(const float *hist_accum, const float *hist_stats, const float *fresh_accum,
                          const float *fresh_stats, int32_t width, int32_t height,
                          const ptmi_validate_params *params, float *out_accum, float *out_stats,
                          float *weight_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_VALIDATE_H */
