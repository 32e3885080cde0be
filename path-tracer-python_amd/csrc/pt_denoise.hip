// pt_denoise.hip — the post-processing ABI (include/ptmi_post.h): a
// variance-guided a-trous filter on the per-pixel error estimates of a stats
// render.
//
//   * dn_load: accum and stats to the working image {r, g, b, v}.
//   * dn_pass<STEP_SMALL>: one a-trous pass (5x5 taps at spacing `step`) with
//     the 3x3 variance prefilter fused, from one working image to the other.
//     STEP_SMALL (steps 1 and 2): the 25-tap footprints of a 16x16 block
//     overlap, so the block stages its pixels plus a 2*step halo in LDS.
//     Otherwise the taps of neighbouring pixels are disjoint and every tap is
//     a 16-byte global load, served by L2 and the Infinity Cache.
//   * dn_store: the working image to out_rgb and out_var.
//
// The arithmetic is pt_denoise_math.hpp's, shared with denoise_check.cpp; the
// kernels only decide where a tap is read from. No cross-lane reads. Not timed
// by ptmi_prof_*, like ptmi_tile_update.
#include <hip/hip_runtime.h>

#include "../../include/ptmi.h"
#include "../../include/ptmi_post.h"
#include "pt_denoise_math.hpp"

namespace ptmi {

int set_last_error(int code, const char* msg);  // pt_abi.hip: the text of ptmi_last_error()

constexpr int kDnBlock = 256;
constexpr int kDnTile = 16;  // a pass block is 16 x 16 pixels
// LDS row stride in pixels: a multiple of 16, so the 16 lanes of a ds_read_b128
// lane group (one pixel column each) hit 16 distinct 16-B slots.
constexpr int kDnLdsStride = 32;
constexpr int kDnLdsRows = kDnTile + 2 * 2 * 2;  // tile plus the halo of step 2

__device__ __forceinline__ DnPx dn_from4(float4 v) {
  DnPx p;
  p.r = v.x;
  p.g = v.y;
  p.b = v.z;
  p.v = v.w;
  return p;
}

__global__ __launch_bounds__(kDnBlock) void dn_load(const float* __restrict__ accum, const float4* __restrict__ stats,
                                                    float4* __restrict__ img, int64_t npix) {
  for (int64_t i = (int64_t)blockIdx.x * kDnBlock + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kDnBlock) {
    const float* a = accum + 3 * i;
    const float4 st = stats[i];
    const DnPx p = dn_load_px(a[0], a[1], a[2], st.x, st.z);
    img[i] = make_float4(p.r, p.g, p.b, p.v);
  }
}

__global__ __launch_bounds__(kDnBlock) void dn_store(const float4* __restrict__ img, float* __restrict__ out_rgb,
                                                     float* __restrict__ out_var, int64_t npix) {
  for (int64_t i = (int64_t)blockIdx.x * kDnBlock + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kDnBlock) {
    const float4 p = img[i];
    float* o = out_rgb + 3 * i;
    o[0] = p.x;
    o[1] = p.y;
    o[2] = p.z;
    if (out_var) out_var[i] = p.w;
  }
}

// One block per 16 x 16 tile, tiles in row-major order over a 1-D grid (an
// image of 1 x 2^31-1 pixels has more tile rows than a grid's y extent).
template <bool STEP_SMALL>
__global__ __launch_bounds__(kDnBlock) void dn_pass(const float4* __restrict__ in, float4* __restrict__ out,
                                                    int32_t width, int32_t height, int32_t tiles_x, int32_t step,
                                                    float sigma) {
  const int32_t ty = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tx = (int32_t)(blockIdx.x - (uint32_t)ty * tiles_x);
  const int32_t x0 = tx * kDnTile, y0 = ty * kDnTile;
  const int32_t x = x0 + (int32_t)(threadIdx.x & (kDnTile - 1)), y = y0 + (int32_t)(threadIdx.x / kDnTile);
  const bool inside = x < width && y < height;
  if (STEP_SMALL) {
    __shared__ float4 tile[kDnLdsRows * kDnLdsStride];
    const int32_t halo = 2 * step, side = kDnTile + 2 * halo;  // side <= kDnLdsRows <= kDnLdsStride
    for (int32_t i = (int32_t)threadIdx.x; i < side * side; i += kDnBlock) {
      const int32_t r = i / side, c = i - r * side;
      const int32_t gx = x0 - halo + c, gy = y0 - halo + r;
      if (gx >= 0 && gx < width && gy >= 0 && gy < height)  // cells outside the image are never read
        tile[r * kDnLdsStride + c] = in[(size_t)gy * (size_t)width + (size_t)gx];
    }
    __syncthreads();
    if (!inside) return;
    const DnPx o = dn_pass_px(x, y, width, height, step, sigma, [&](int32_t qx, int32_t qy) {
      return dn_from4(tile[(qy - y0 + halo) * kDnLdsStride + (qx - x0 + halo)]);
    });
    out[(size_t)y * (size_t)width + (size_t)x] = make_float4(o.r, o.g, o.b, o.v);
  } else {
    if (!inside) return;
    const DnPx o = dn_pass_px(x, y, width, height, step, sigma, [&](int32_t qx, int32_t qy) {
      return dn_from4(in[(size_t)qy * (size_t)width + (size_t)qx]);
    });
    out[(size_t)y * (size_t)width + (size_t)x] = make_float4(o.r, o.g, o.b, o.v);
  }
}

// Which passes take the LDS form: steps up to this one (0: none). Steps 1 and
// 2 by default; the setter exists for the A/B record of profiles/denoise.
static int32_t g_lds_max_step = 2;

static hipError_t launch_denoise(const float* accum, const float* stats, int32_t width, int32_t height,
                                 int32_t iterations, float sigma, void* ws, float* out_rgb, float* out_var,
                                 hipStream_t stream) {
  const int64_t npix = (int64_t)width * height;
  float4* buf[2] = {(float4*)ws, (float4*)ws + npix};
  const int64_t nb = (npix + kDnBlock - 1) / kDnBlock;
  const dim3 flat((unsigned)(nb > 4096 ? 4096 : nb));
  hipLaunchKernelGGL(dn_load, flat, dim3(kDnBlock), 0, stream, accum, (const float4*)stats, buf[0], npix);
  const int32_t tiles_x = (width + kDnTile - 1) / kDnTile;
  const int64_t tiles = (int64_t)tiles_x * ((height + kDnTile - 1) / kDnTile);  // <= 2^31-1 pixels / 16 + rows
  int cur = 0;
  for (int32_t i = 0; i < iterations; ++i) {
    const int32_t step = 1 << i;
    if (step <= g_lds_max_step)
      hipLaunchKernelGGL(dn_pass<true>, dim3((unsigned)tiles), dim3(kDnBlock), 0, stream, buf[cur], buf[cur ^ 1],
                         width, height, tiles_x, step, sigma);
    else
      hipLaunchKernelGGL(dn_pass<false>, dim3((unsigned)tiles), dim3(kDnBlock), 0, stream, buf[cur], buf[cur ^ 1],
                         width, height, tiles_x, step, sigma);
    cur ^= 1;
  }
  hipLaunchKernelGGL(dn_store, flat, dim3(kDnBlock), 0, stream, buf[cur], out_rgb, out_var, npix);
  return hipGetLastError();
}

}  // namespace ptmi

using namespace ptmi;

static int64_t dn_pixels(int32_t width, int32_t height) {
  if (width < 1 || height < 1) return 0;
  const int64_t n = (int64_t)width * (int64_t)height;
  return n > 0x7fffffff ? 0 : n;
}

extern "C" {

size_t ptmi_denoise_workspace_bytes(int32_t width, int32_t height) {
  const int64_t npix = dn_pixels(width, height);
  if (npix == 0) {
    set_last_error(PTMI_EINVAL, "denoise: bad image size (width and height >= 1, at most 2^31-1 pixels)");
    return 0;
  }
  return dn_workspace_bytes(npix);
}

int ptmi_denoise(const float* accum, const float* stats, int32_t width, int32_t height, int32_t iterations,
                 float sigma, void* workspace, size_t workspace_bytes, float* out_rgb, float* out_var, void* stream) {
  if (!accum) return set_last_error(PTMI_EINVAL, "denoise: accum is NULL");
  if (!stats || ((uintptr_t)stats & 15u)) return set_last_error(PTMI_EINVAL, "denoise: stats NULL/misaligned");
  if (!workspace || ((uintptr_t)workspace & 15u))
    return set_last_error(PTMI_EINVAL, "denoise: workspace NULL/misaligned");
  if (!out_rgb) return set_last_error(PTMI_EINVAL, "denoise: out_rgb is NULL");
  const int64_t npix = dn_pixels(width, height);
  if (npix == 0)
    return set_last_error(PTMI_EINVAL, "denoise: bad image size (width and height >= 1, at most 2^31-1 pixels)");
  if (iterations < 0 || iterations > kDnMaxIterations)
    return set_last_error(PTMI_EINVAL, "denoise: iterations must be in [0, 8]");
  if (!(sigma >= 0.0f)) return set_last_error(PTMI_EINVAL, "denoise: sigma must be >= 0");
  if (workspace_bytes < dn_workspace_bytes(npix)) return set_last_error(PTMI_EINVAL, "denoise: workspace too small");
  const uintptr_t a = (uintptr_t)accum, o = (uintptr_t)out_rgb, bytes = (uintptr_t)(12 * npix);
  if (a < o + bytes && o < a + bytes) return set_last_error(PTMI_EINVAL, "denoise: out_rgb aliases accum");
  const hipError_t e =
      launch_denoise(accum, stats, width, height, iterations, sigma, workspace, out_rgb, out_var, (hipStream_t)stream);
  if (e != hipSuccess) {
    set_last_error(PTMI_EHIP, hipGetErrorString(e));
    return PTMI_EHIP;
  }
  return PTMI_OK;
}

int ptmi_denoise_set_lds_max_step(int32_t max_step) {
  if (max_step < 0 || max_step > 2) return set_last_error(PTMI_EINVAL, "denoise: the LDS form covers steps 1 and 2");
  const int32_t prev = g_lds_max_step;
  g_lds_max_step = max_step;
  return prev;
}

}  // extern "C"
