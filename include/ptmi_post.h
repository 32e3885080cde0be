/*
 * ptmi_post.h — the post-processing ABI of libptmi.so: what runs on a finished
 * accumulator, after the integrator of ptmi.h. It is versioned apart from
 * PTMI_ABI_VERSION: nothing in ptmi.h changes with it. Error codes and
 * ptmi_last_error() are ptmi.h's. Version 1: a variance-guided a-trous
 * denoiser on the per-pixel error estimates of a stats render (ptmi.h, ABI
 * v8: stats[pixel] = {n, mean, M2, reserved} of the sample luminance).
 *
 * The filter. All arithmetic is f32 with one rounding per operation
 * (-ffp-contract=off, correctly rounded / and sqrtf) and no transcendentals,
 * so numpy f32 reproduces every output bit for bit. The image is width x
 * height and whole (no windows, no bands), on one device.
 *
 * Input per pixel p: n = stats[p][0]; scale = (float)(1.0 / (double)max(n, 1))
 * as in ptmi_tonemap_stats; c_p = accum[p] * scale per channel;
 * l_p = (0.2126f*r + 0.7152f*g) + 0.0722f*b of c_p; the variance of the mean
 * luminance v_p = (M2 / (n - 1)) / n for n >= 2, else 1e10f ("unknown: trust
 * the neighbours").
 *
 * A pixel is invalid if l_p or v_p is not finite (!(fabsf(x) <= FLT_MAX)), as a
 * pass reads it. Invalid pixels are copied through every pass unchanged and
 * have weight 0 wherever they appear as a tap: a NaN sample stays one NaN
 * pixel, as in the tone map.
 *
 * Two ping-pong images of float4 {r, g, b, v} live in the workspace; l is
 * recomputed from the current colour in each pass.
 *
 * Pass i = 0 .. iterations-1, step s = 1 << i, for every valid pixel p:
 *  1. Prefiltered variance, used only in the edge-stopping term:
 *     vbar_p = (sum g(dx)*g(dy)*v_q) / (sum g(dx)*g(dy)) over the 3x3 taps
 *     q = p + (dx, dy) at unit spacing whatever s is, dy the outer loop, both
 *     ascending, taps inside the image and valid only; g = {1/2, 1/4} for
 *     |d| = 0, 1; products formed as (g(dx)*g(dy))*v_q, sums sequential f32
 *     adds in tap order.
 *  2. den = sigma * sqrtf(vbar_p) + 1e-4f.
 *  3. 5x5 taps q = p + s*(dx, dy), dy outer, dx inner, both -2 .. 2 ascending;
 *     taps outside the image or invalid are skipped. h = k[|dx|] * k[|dy|],
 *     k = {0.375f, 0.25f, 0.0625f}; x = fabsf(l_p - l_q) / den;
 *     t = fmaxf(0.0f, 1.0f - x); w = h * (t * t). C += w * c_q per channel,
 *     V += (w * w) * v_q, W += w: sequential adds in tap order.
 *  4. c'_p = C / W per channel, v'_p = V / (W * W). The centre tap has
 *     w = 0.140625f, so W > 0.
 *
 * After the last pass out_rgb[p] = c_p (height x width x 3 f32) and, if
 * out_var is not NULL, out_var[p] = v_p: the variance the filter claims for
 * the result. iterations == 0 returns the inputs of pass 0. The 8-bit image is
 * ptmi_tonemap(out_rgb, u8, width, height, spp = 1).
 */
#ifndef PTMI_POST_H
#define PTMI_POST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_POST_VERSION 1

/* Bytes of the workspace of ptmi_denoise: 2 * 16 B * pixels, rounded up to
 * 256; 0 (and a message) for width or height < 1 or more than 2^31-1 pixels. */
size_t ptmi_denoise_workspace_bytes(int32_t width, int32_t height);

/* The filter above: dn_load, `iterations` launches of dn_pass, dn_store.
 * Asynchronous on `stream`, graph-capturable, no allocation, not timed by
 * ptmi_prof_*. PTMI_EINVAL, each with a message and before any HIP call: a
 * NULL accum, stats, workspace or out_rgb; stats or workspace not 16-byte
 * aligned; width or height < 1, or more than 2^31-1 pixels; iterations
 * outside 0 .. 8; sigma negative or NaN; workspace_bytes below
 * ptmi_denoise_workspace_bytes; out_rgb overlapping accum. out_var may be
 * NULL. */
int ptmi_denoise(const float *accum, const float *stats, int32_t width, int32_t height, int32_t iterations,
                 float sigma, void *workspace, size_t workspace_bytes, float *out_rgb, float *out_var,
                 void *stream);

/* Which passes stage their taps in LDS: those of step <= max_step (0: none;
 * default and maximum 2). The other passes read every tap from global memory;
 * both forms compute the same bits. For A/B timing; returns the previous
 * value, PTMI_EINVAL outside 0 .. 2. Process-wide. */
int ptmi_denoise_set_lds_max_step(int32_t max_step);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_POST_H */
