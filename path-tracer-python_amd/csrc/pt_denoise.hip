// pt_denoise.hip — the a-trous filter of the post-processing ABI
// (include/ptmi_post.h, DESIGN.md §13: variance-guided, on the per-pixel error
// estimates of a stats render) and of the guide ABI (include/ptmi_guide.h,
// guided by the first-hit guide buffers as well). One set of
// kernels, GUIDED at compile time.
//
//   * dn_load<GUIDED>: accum and stats to the working image {r, g, b, v};
//     GUIDED with the albedo demodulation.
//   * dn_pass<STEP_SMALL, GUIDED>: one a-trous pass (5x5 taps at spacing
//     `step`) with the 3x3 variance prefilter fused, from one working image to
//     the other. STEP_SMALL (steps 1 and 2): the 25-tap footprints of a 16x16
//     block overlap, so the block stages its pixels plus a 2*step halo in LDS.
//     Otherwise the taps of neighbouring pixels are disjoint and every tap is
//     a 16-byte global load, served by L2 and the Infinity Cache. A GUIDED tap
//     is 48 B: the working pixel and the two halves of its guide pixel, which
//     both forms read from global memory (L2-resident). Staging the guides in
//     LDS as well (three 16-B planes, 36 KiB per block) was built and timed
//     and is no faster: not kept.
//   * dn_store<GUIDED>: the working image to out_rgb and out_var.
//
// The arithmetic is pt_denoise_math.hpp's, shared with denoise_check.cpp; the
// kernels only decide where a tap is read from. No cross-lane reads. Not timed
// by ptmi_prof_*, like ptmi_tile_update.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_guide.h"
#include "../../include/ptmi_post.h"
#include "pt_args.hpp"
#include "pt_image.hpp"

namespace ptmi {

// LDS row stride in pixels: a multiple of 16, so the 16 lanes of a ds_read_b128
// lane group (one pixel column each) hit 16 distinct 16-B slots.
constexpr int kDnLdsStride = 32;
constexpr int kDnLdsRows = kImgTile + 2 * 2 * 2;  // tile plus the halo of step 2

template <bool GUIDED>
__global__ __launch_bounds__(kImgBlock) void dn_load(const float* __restrict__ accum, const float4* __restrict__ stats,
                                                     const float4* __restrict__ guides, float4* __restrict__ img,
                                                     int64_t npix, int32_t demodulate) {
  for (int64_t i = (int64_t)blockIdx.x * kImgBlock + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kImgBlock) {
    const float* a = accum + 3 * i;
    const float4 st = stats[i];
    DngG g = {};
    if (GUIDED && demodulate) g = load_guide(guides, (size_t)i);
    img[i] = px_to4(dng_load_px(a[0], a[1], a[2], st.x, st.z, g, GUIDED ? demodulate : 0));
  }
}

template <bool GUIDED>
__global__ __launch_bounds__(kImgBlock) void dn_store(const float4* __restrict__ img, const float4* __restrict__ guides,
                                                      float* __restrict__ out_rgb, float* __restrict__ out_var,
                                                      int64_t npix, int32_t demodulate) {
  for (int64_t i = (int64_t)blockIdx.x * kImgBlock + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kImgBlock) {
    DngG g = {};
    if (GUIDED && demodulate) g = load_guide(guides, (size_t)i);
    const DnPx p = dng_store_px(px_from4(img[i]), g, GUIDED ? demodulate : 0);
    float* o = out_rgb + 3 * i;
    o[0] = p.r;
    o[1] = p.g;
    o[2] = p.b;
    if (out_var) out_var[i] = p.v;
  }
}

template <bool STEP_SMALL, bool GUIDED>
__global__ __launch_bounds__(kImgBlock) void dn_pass(const float4* __restrict__ in, const float4* __restrict__ guides,
                                                     float4* __restrict__ out, int32_t width, int32_t height,
                                                     int32_t tiles_x, int32_t step, DngParams prm) {
  const TileXY t = tile_xy<kImgTile>(tiles_x);
  const bool inside = t.x < width && t.y < height;
  auto index = [&](int32_t qx, int32_t qy) { return (size_t)qy * (size_t)width + (size_t)qx; };
  auto guide = [&](int32_t qx, int32_t qy) { return load_guide(guides, index(qx, qy)); };
  if (STEP_SMALL) {
    __shared__ float4 tile[kDnLdsRows * kDnLdsStride];
    const int32_t halo = 2 * step, side = kImgTile + 2 * halo;  // side <= kDnLdsRows <= kDnLdsStride
    for (int32_t i = (int32_t)threadIdx.x; i < side * side; i += kImgBlock) {
      const int32_t r = i / side, c = i - r * side;
      const int32_t gx = t.x0 - halo + c, gy = t.y0 - halo + r;
      if (gx >= 0 && gx < width && gy >= 0 && gy < height)  // cells outside the image are never read
        tile[r * kDnLdsStride + c] = in[index(gx, gy)];
    }
    __syncthreads();
    if (!inside) return;
    out[index(t.x, t.y)] = px_to4(dn_pass_px<GUIDED>(
        t.x, t.y, width, height, step, prm,
        [&](int32_t qx, int32_t qy) {
          return px_from4(tile[(qy - t.y0 + halo) * kDnLdsStride + (qx - t.x0 + halo)]);
        },
        guide));
  } else {
    if (!inside) return;
    out[index(t.x, t.y)] = px_to4(dn_pass_px<GUIDED>(
        t.x, t.y, width, height, step, prm, [&](int32_t qx, int32_t qy) { return px_from4(in[index(qx, qy)]); },
        guide));
  }
}

// Which passes take the LDS form: steps up to this one (0: none), one switch
// per mode. Steps 1 and 2 by default; the setters exist for the A/B records of
// profiles/denoise and profiles/guided.
static int32_t g_lds_max_step[2] = {2, 2};  // [GUIDED]

// guides = nullptr for the unguided filter, which reads prm.sigma only.
template <bool GUIDED>
static hipError_t launch_denoise(const float* accum, const float* stats, const float* guides, int32_t width,
                                 int32_t height, int32_t iterations, const DngParams& prm, void* ws, float* out_rgb,
                                 float* out_var, hipStream_t stream) {
  const int64_t npix = (int64_t)width * height;
  float4* buf[2] = {(float4*)ws, (float4*)ws + npix};
  const float4* g4 = (const float4*)guides;
  const dim3 flat = capped_grid(npix, kImgBlock), block(kImgBlock);
  hipLaunchKernelGGL(dn_load<GUIDED>, flat, block, 0, stream, accum, (const float4*)stats, g4, buf[0], npix,
                     prm.demodulate);
  const int32_t tiles_x = image_tiles_x(width, kImgTile);
  const dim3 tiles = image_tile_grid(width, height, kImgTile);
  int cur = 0;
  for (int32_t i = 0; i < iterations; ++i) {
    const int32_t step = 1 << i;
    if (step <= g_lds_max_step[GUIDED])
      hipLaunchKernelGGL((dn_pass<true, GUIDED>), tiles, block, 0, stream, buf[cur], g4, buf[cur ^ 1], width, height,
                         tiles_x, step, prm);
    else
      hipLaunchKernelGGL((dn_pass<false, GUIDED>), tiles, block, 0, stream, buf[cur], g4, buf[cur ^ 1], width, height,
                         tiles_x, step, prm);
    cur ^= 1;
  }
  hipLaunchKernelGGL(dn_store<GUIDED>, flat, block, 0, stream, buf[cur], g4, out_rgb, out_var, npix, prm.demodulate);
  return hipGetLastError();
}

static int set_lds_max_step(bool guided, int32_t max_step) {
  if (max_step < 0 || max_step > 2)
    return fail(PTMI_EINVAL, "%s: the LDS form covers steps 1 and 2", guided ? "denoise_guided" : "denoise");
  const int32_t prev = g_lds_max_step[guided];
  g_lds_max_step[guided] = max_step;
  return prev;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

size_t ptmi_denoise_workspace_bytes(int32_t width, int32_t height) {
  const int64_t npix = image_pixels(width, height);
  if (npix == 0) {
    fail(PTMI_EINVAL, "denoise: bad image size (width and height >= 1, at most 2^31-1 pixels)");
    return 0;
  }
  return dn_workspace_bytes(npix);
}

int ptmi_denoise(const float* accum, const float* stats, int32_t width, int32_t height, int32_t iterations,
                 float sigma, void* workspace, size_t workspace_bytes, float* out_rgb, float* out_var, void* stream) {
  if (!accum) return fail(PTMI_EINVAL, "denoise: accum is NULL");
  if (bad16(stats)) return fail(PTMI_EINVAL, "denoise: stats NULL/misaligned");
  if (bad16(workspace)) return fail(PTMI_EINVAL, "denoise: workspace NULL/misaligned");
  if (!out_rgb) return fail(PTMI_EINVAL, "denoise: out_rgb is NULL");
  const int64_t npix = image_pixels(width, height);
  if (npix == 0) return fail(PTMI_EINVAL, "denoise: bad image size (width and height >= 1, at most 2^31-1 pixels)");
  if (iterations < 0 || iterations > kDnMaxIterations)
    return fail(PTMI_EINVAL, "denoise: iterations must be in [0, 8]");
  if (!(sigma >= 0.0f)) return fail(PTMI_EINVAL, "denoise: sigma must be >= 0");
  if (workspace_bytes < dn_workspace_bytes(npix)) return fail(PTMI_EINVAL, "denoise: workspace too small");
  const uint64_t n = (uint64_t)npix;
  if (overlaps(out_rgb, 12 * n, accum, 12 * n)) return fail(PTMI_EINVAL, "denoise: out_rgb aliases accum");
  DngParams prm = {};
  prm.sigma = sigma;
  return hip_result(launch_denoise<false>(accum, stats, nullptr, width, height, iterations, prm, workspace, out_rgb,
                                          out_var, (hipStream_t)stream));
}

int ptmi_denoise_set_lds_max_step(int32_t max_step) { return set_lds_max_step(false, max_step); }

int ptmi_denoise_guided(const float* accum, const float* stats, const float* guides, int32_t width, int32_t height,
                        const ptmi_dn_guided_params* params, void* workspace, size_t workspace_bytes, float* out_rgb,
                        float* out_var, void* stream) {
  if (!accum) return fail(PTMI_EINVAL, "denoise_guided: accum is NULL");
  if (bad16(stats)) return fail(PTMI_EINVAL, "denoise_guided: stats NULL/misaligned");
  if (bad16(guides)) return fail(PTMI_EINVAL, "denoise_guided: guides NULL/misaligned");
  if (!params) return fail(PTMI_EINVAL, "denoise_guided: params is NULL");
  if (bad16(workspace)) return fail(PTMI_EINVAL, "denoise_guided: workspace NULL/misaligned");
  if (!out_rgb) return fail(PTMI_EINVAL, "denoise_guided: out_rgb is NULL");
  const int64_t npix = image_pixels(width, height);
  if (npix == 0)
    return fail(PTMI_EINVAL, "denoise_guided: bad image size (width and height >= 1, at most 2^31-1 pixels)");
  if (params->iterations < 0 || params->iterations > kDnMaxIterations)
    return fail(PTMI_EINVAL, "denoise_guided: iterations must be in [0, 8]");
  if (!(params->sigma >= 0.0f)) return fail(PTMI_EINVAL, "denoise_guided: sigma must be >= 0");
  if (!(params->sigma_z >= 0.0f)) return fail(PTMI_EINVAL, "denoise_guided: sigma_z must be >= 0");
  if (!(params->sigma_a >= 0.0f)) return fail(PTMI_EINVAL, "denoise_guided: sigma_a must be >= 0");
  if (params->normal_power_log2 < 0 || params->normal_power_log2 > kDngMaxNormalPower)
    return fail(PTMI_EINVAL, "denoise_guided: normal_power_log2 must be in [0, 7]");
  if (params->flags & ~PTMI_DN_DEMODULATE) return fail(PTMI_EINVAL, "denoise_guided: unknown flag bits");
  if (workspace_bytes < dn_workspace_bytes(npix)) return fail(PTMI_EINVAL, "denoise_guided: workspace too small");
  const uint64_t n = (uint64_t)npix;
  if (overlaps(out_rgb, 12 * n, accum, 12 * n)) return fail(PTMI_EINVAL, "denoise_guided: out_rgb aliases accum");
  if (overlaps(out_rgb, 12 * n, stats, 16 * n)) return fail(PTMI_EINVAL, "denoise_guided: out_rgb aliases stats");
  if (overlaps(out_rgb, 12 * n, guides, 32 * n)) return fail(PTMI_EINVAL, "denoise_guided: guides aliases out_rgb");
  if (out_var && overlaps(out_var, 4 * n, guides, 32 * n))
    return fail(PTMI_EINVAL, "denoise_guided: guides aliases out_var");
  DngParams prm;
  prm.sigma = params->sigma;
  prm.sigma_z = params->sigma_z;
  prm.sigma_a = params->sigma_a;
  prm.normal_power_log2 = params->normal_power_log2;
  prm.demodulate = (params->flags & PTMI_DN_DEMODULATE) ? 1 : 0;
  return hip_result(launch_denoise<true>(accum, stats, guides, width, height, params->iterations, prm, workspace,
                                         out_rgb, out_var, (hipStream_t)stream));
}

int ptmi_denoise_guided_set_lds_max_step(int32_t max_step) { return set_lds_max_step(true, max_step); }

}  // extern "C"
