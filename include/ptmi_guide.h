/*
 * ptmi_guide.h — the guide ABI of libptmi.so: first-hit guide buffers (normal,
 * depth, albedo) from one deterministic primary ray per pixel, and the a-trous
 * denoiser of ptmi_post.h with those guides as further edge-stopping terms. It
 * is versioned apart from PTMI_ABI_VERSION and PTMI_POST_VERSION: nothing in
 * ptmi.h or ptmi_post.h changes with it. Error codes, ptmi_last_error(),
 * ptmi_scene_view and ptmi_frame are ptmi.h's; the workspace is
 * ptmi_denoise's (ptmi_denoise_workspace_bytes, ptmi_post.h).
 *
 * All arithmetic is f32 with one rounding per operation (-ffp-contract=off,
 * correctly rounded / and sqrtf), in the order written here. Guides are
 * whole-frame and single-device, like the denoiser.
 *
 * ---- The guide image
 *
 * guides[height][width][8] f32, 32 bytes per pixel:
 *   {nx, ny, nz, depth, ar, ag, ab, hit}.
 *
 * ---- The guide trace (ptmi_guide_trace)
 *
 * One primary ray per pixel (px, py); nothing is drawn from the RNG.
 *   ps = (pixel00 + delta_u * (float)px) + delta_v * (float)py   (get_ray with
 *        both jitter offsets 0, same operation order);
 *   o = center (no defocus); d = ps - o, not normalised;
 *   len = sqrtf(dot(d, d)), dot = (x*x + y*y) + z*z; z = 0.
 * Up to 4 traversals, each the closest hit of traverse(o, d, 0.001f, 1e10f)
 * with the frame's traversal mode:
 *   - no hit: the pixel is a miss;
 *   - a hit at t: hp = o + d * t, z = z + t * len. If the primitive's material
 *     row has the constant-medium flag, o = hp and the next traversal starts
 *     there; a medium hit in the fourth traversal makes the pixel a miss. So a
 *     medium boundary is seen through, with no random decision.
 * A surface hit writes n = hit_normal (the sphere's (hp - c) / r; a quad's or
 * triangle's stored normal, turned against d), depth = z, hit = 1.0f and the
 * albedo: the material's texture at hp for material types 0 (lambertian) and 4
 * (isotropic), the metal colour for type 1, (1, 1, 1) for every other type
 * (dielectric, emissive, unknown). A miss writes n = 0, depth = 1e10f, albedo
 * (1, 1, 1), hit = 0.0f.
 *
 * Not averaged over the pixel or the lens; a mirror or glass pixel reports the
 * mirror or the glass.
 *
 * ---- The guided filter (ptmi_denoise_guided)
 *
 * ptmi_denoise's contract (ptmi_post.h) with the changes below; everything not
 * mentioned is unchanged: validity, the 3x3 prefiltered variance, den, tap
 * order, sequential sums, invalid pixels copied through. The guides of a pixel
 * are the same in every pass.
 *
 * Load: c_p, v_p as ptmi_denoise loads them. With PTMI_DN_DEMODULATE, per
 * channel m = fmaxf(a, 0.0f) + 1e-3f from the pixel's guide albedo, c = c / m;
 * lm = (0.2126f*m_r + 0.7152f*m_g) + 0.0722f*m_b; v = v / (lm * lm).
 *
 * Tap weight, p the centre and q the tap, h and t as in ptmi_denoise:
 *   tz = fmaxf(0, 1 - fabsf(z_p - z_q) / (sigma_z * z_p + 1e-4f))
 *   da = (|ar_p - ar_q| + |ag_p - ag_q|) + |ab_p - ab_q|
 *   ta = fmaxf(0, 1 - da / (sigma_a + 1e-4f))
 *   dn = fminf(1, fmaxf(0, (nx_p*nx_q + ny_p*ny_q) + nz_p*nz_q)), then
 *        dn = dn * dn, normal_power_log2 times
 *   wn = dn if both pixels have hit != 0, 1.0f if both have hit == 0, else 0.0f
 *   w  = ((h * (t * t)) * (tz * tz)) * ((ta * ta) * wn)
 * For the centre tap t = tz = ta = 1 exactly (the differences are 0, for finite
 * guides) and wn is 1.0f on a miss and dn on a hit: the squared length of the
 * pixel's own normal, a unit vector up to rounding, clamped to 1 and squared at
 * most 7 times, which stays far above 0. So W > 0 still holds for guides as
 * ptmi_guide_trace writes them. Guides from elsewhere must be finite, with
 * unit normals on hit pixels.
 *
 * Store: out_rgb = c, out_var = v; with PTMI_DN_DEMODULATE out_rgb = c * m per
 * channel and out_var = v * (lm * lm). So with the flag, iterations == 0
 * returns (c / m) * m, which is c only up to two roundings, and v likewise.
 */
#ifndef PTMI_GUIDE_H
#define PTMI_GUIDE_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_GUIDE_VERSION 1

#define PTMI_DN_DEMODULATE 1 /* ptmi_dn_guided_params.flags, bit 0 */

/* The guide trace above: one kernel, one lane per pixel, one wave per 8x8
 * pixel square. Asynchronous on `stream`, graph-capturable, no allocation, not
 * timed by ptmi_prof_*. PTMI_EINVAL, each with a message and before any HIP
 * call: whatever a render call rejects in scene and frame; a NULL guides or
 * one not 16-byte aligned; a frame that is windowed (x0, y0, w, h not the
 * whole image) or banded (band_stride != 1). */
int ptmi_guide_trace(const ptmi_scene_view *scene, const ptmi_frame *frame, float *guides, void *stream);

typedef struct ptmi_dn_guided_params {
    int32_t iterations;        /* 0 .. 8 */
    float sigma;               /* luminance term, as ptmi_denoise */
    float sigma_z;             /* relative depth */
    float sigma_a;             /* albedo, L1 over rgb */
    int32_t normal_power_log2; /* 0 .. 7: the clamped normal dot product is squared this many times */
    int32_t flags;             /* bit 0: PTMI_DN_DEMODULATE; other bits must be 0 */
} ptmi_dn_guided_params;

/* The guided filter above: dn_load, `iterations` launches of dn_pass,
 * dn_store (their GUIDED forms); the guides are read in place. Asynchronous on `stream`,
 * graph-capturable, no allocation, not timed by ptmi_prof_*. PTMI_EINVAL, each
 * with a message and before any HIP call: every case ptmi_denoise rejects
 * (ptmi_post.h; iterations and sigma are the params'); a NULL guides or
 * params; guides not 16-byte aligned; guides overlapping out_rgb or out_var;
 * out_rgb overlapping accum or stats; sigma_z or sigma_a negative or NaN;
 * normal_power_log2 outside 0 .. 7; unknown flag bits. out_var may be NULL. */
int ptmi_denoise_guided(const float *accum, const float *stats, const float *guides, int32_t width, int32_t height,
                        const ptmi_dn_guided_params *params, void *workspace, size_t workspace_bytes,
                        float *out_rgb, float *out_var, void *stream);

/* Which guided passes stage their colour taps in LDS: those of step <= max_step
 * (0: none; default and maximum 2). The other passes read every tap from global
 * memory, and every pass reads a tap's guides from global memory; both forms
 * compute the same bits. For A/B timing; returns the previous value,
 * PTMI_EINVAL outside 0 .. 2. Process-wide, and apart from
 * ptmi_denoise_set_lds_max_step. */
int ptmi_denoise_guided_set_lds_max_step(int32_t max_step);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_GUIDE_H */
