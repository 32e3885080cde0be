// pt_guide.hip — the guide ABI (include/ptmi_guide.h): first-hit guide buffers
// and the a-trous denoiser guided by them.
//
//   * guide_trace<STACK, TRAV>: one deterministic primary ray per pixel, one
//     lane per pixel, one wave (one block) per 8x8 pixel square, so a wave's
//     rays are coherent. Up to 4 traversals per lane (medium boundaries are
//     seen through); the LDS stack is the render kernels'. Each 32-byte guide
//     pixel is written as two 16-B stores. No cross-lane reads beyond those
//     inside traverse()'s leaf tests.
//   * dng_load / dng_store: dn_load / dn_store with the albedo demodulation.
//   * dng_pass<STEP_SMALL>: one guided a-trous pass. A tap is 48 B: the working
//     pixel and the two halves of its guide pixel. STEP_SMALL (steps 1 and 2)
//     stages the working pixels of the block's halo tile in LDS, as dn_pass,
//     and reads a tap's guides from global memory (L2-resident); larger steps
//     read all of a tap from global memory. Staging the guides in LDS as well
//     (three 16-B planes, 36 KiB per block) was built and timed and is no
//     faster: not kept.
//
// The filter's arithmetic is pt_guide_math.hpp's, shared with guide_check.cpp;
// the kernels only decide where a tap is read from. pt_denoise.hip and its
// kernels are not involved. Not timed by ptmi_prof_*.
#include <hip/hip_runtime.h>

#include "../../include/ptmi.h"
#include "../../include/ptmi_guide.h"
#include "pt_guide_math.hpp"
#include "pt_launch.hpp"

namespace ptmi {

int set_last_error(int code, const char* msg);  // pt_abi.hip: the text of ptmi_last_error()
// pt_abi.hip: a render call's scene and frame checks and conversion; slots = stack slots needed
int guide_to_dev(const ptmi_scene_view* scene, const ptmi_frame* frame, DevScene& sc, DevFrame& fr, int32_t& slots);

// ---------------------------------------------------------------- the guide trace
constexpr int kGuideBlock = 64;  // one wave: an 8 x 8 pixel square
constexpr int kGuideSquare = 8;
constexpr int kGuideTraversals = 4;
constexpr float kGuideMissDepth = 1e10f;

template <int STACK, int TRAV>
__global__ __launch_bounds__(kGuideBlock, stress_waves(1)) void guide_trace(DevScene sc, DevFrame fr,
                                                                            float4* __restrict__ guides,
                                                                            int32_t squares_x) {
  __shared__ uint2 lds_stack[STACK * kGuideBlock];
  const int tid = threadIdx.x;
  Stack st{lds_stack + tid};
  const int32_t sy = (int32_t)(blockIdx.x / (uint32_t)squares_x), sx = (int32_t)(blockIdx.x - (uint32_t)sy * squares_x);
  const int32_t px = sx * kGuideSquare + (tid & (kGuideSquare - 1)), py = sy * kGuideSquare + (tid / kGuideSquare);
  if (px >= fr.width || py >= fr.height) return;

  // get_ray (pt_device.hpp) with both jitter offsets 0 and no defocus
  const pt_v3 p00 = pt_v3f(fr.pixel00[0], fr.pixel00[1], fr.pixel00[2]);
  const pt_v3 du = pt_v3f(fr.delta_u[0], fr.delta_u[1], fr.delta_u[2]);
  const pt_v3 dv = pt_v3f(fr.delta_v[0], fr.delta_v[1], fr.delta_v[2]);
  const pt_v3 ps = pt_add(pt_add(p00, pt_scale(du, (float)px)), pt_scale(dv, (float)py));
  pt_v3 o = pt_v3f(fr.center[0], fr.center[1], fr.center[2]);
  const pt_v3 d = pt_sub(ps, o);
  const float len = sqrtf(pt_dot(d, d));

  float z = 0.0f;
  bool surface = false;
  int32_t ref = 0, g = 0;
  pt_v3 hp = o;
  for (int k = 0; k < kGuideTraversals; ++k) {
    float t = 0.0f;
    if (!traverse<STACK, kGuideBlock, TRAV>(sc, o, d, kTMin, kTMax, st, t, ref)) break;
    hp = pt_add(o, pt_scale(d, t));
    z = z + t * len;
    g = mat_index(sc, ref);
    if (!((mat_flags(sc, g) >> 8) & 1u)) {
      surface = true;
      break;
    }
    o = hp;  // a medium boundary: look through it
  }

  float4 gn = make_float4(0.0f, 0.0f, 0.0f, kGuideMissDepth), ga = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
  if (surface) {
    const pt_v3 n = hit_normal(sc, ref, hp, d);
    const Mat m = load_mat(sc, g);
    const int32_t mt = m.mat_type();
    pt_v3 a = pt_v3f(1.0f, 1.0f, 1.0f);
    if (mt == 0 || mt == 4)
      a = eval_texture(sc, ref, m, hp);
    else if (mt == 1)
      a = pt_v3f(m.m0.x, m.m0.y, m.m0.z);
    gn = make_float4(n.x, n.y, n.z, z);
    ga = make_float4(a.x, a.y, a.z, 1.0f);
  }
  const size_t p = (size_t)py * (size_t)fr.width + (size_t)px;
  guides[2 * p] = gn;
  guides[2 * p + 1] = ga;
}

static hipError_t launch_guide_trace(const DevScene& sc, const DevFrame& fr, int32_t stack_needed, float* guides,
                                     hipStream_t stream) {
  const int32_t squares_x = (fr.width + kGuideSquare - 1) / kGuideSquare;
  const int64_t squares = (int64_t)squares_x * ((fr.height + kGuideSquare - 1) / kGuideSquare);  // < 2^31 / 3 pixels / 64 + edges
  return dispatch_traversal<false>(fr, stack_needed, [&](auto stack, auto trav) {
    constexpr int S = decltype(stack)::value, T = decltype(trav)::value;
    hipLaunchKernelGGL((guide_trace<S, T>), dim3((unsigned)squares), dim3(kGuideBlock), 0, stream, sc, fr,
                       (float4*)guides, squares_x);
    return hipGetLastError();
  });
}

// ---------------------------------------------------------------- the guided filter
constexpr int kDngBlock = 256;
constexpr int kDngTile = 16;  // a pass block is 16 x 16 pixels
// LDS row stride in pixels: a multiple of 16, so the 16 lanes of a ds_read_b128
// lane group (one pixel column each) hit 16 distinct 16-B slots (as dn_pass).
constexpr int kDngLdsStride = 32;
constexpr int kDngLdsRows = kDngTile + 2 * 2 * 2;  // tile plus the halo of step 2

__device__ __forceinline__ DnPx dng_from4(float4 v) {
  DnPx p;
  p.r = v.x;
  p.g = v.y;
  p.b = v.z;
  p.v = v.w;
  return p;
}

__device__ __forceinline__ DngG dng_guide(float4 n, float4 a) {
  DngG g;
  g.nx = n.x;
  g.ny = n.y;
  g.nz = n.z;
  g.z = n.w;
  g.ar = a.x;
  g.ag = a.y;
  g.ab = a.z;
  g.hit = a.w;
  return g;
}

__global__ __launch_bounds__(kDngBlock) void dng_load(const float* __restrict__ accum, const float4* __restrict__ stats,
                                                      const float4* __restrict__ guides, float4* __restrict__ img,
                                                      int64_t npix, int32_t demodulate) {
  for (int64_t i = (int64_t)blockIdx.x * kDngBlock + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kDngBlock) {
    const float* a = accum + 3 * i;
    const float4 st = stats[i];
    DngG g = {};
    if (demodulate) g = dng_guide(guides[2 * i], guides[2 * i + 1]);
    const DnPx p = dng_load_px(a[0], a[1], a[2], st.x, st.z, g, demodulate);
    img[i] = make_float4(p.r, p.g, p.b, p.v);
  }
}

__global__ __launch_bounds__(kDngBlock) void dng_store(const float4* __restrict__ img, const float4* __restrict__ guides,
                                                       float* __restrict__ out_rgb, float* __restrict__ out_var,
                                                       int64_t npix, int32_t demodulate) {
  for (int64_t i = (int64_t)blockIdx.x * kDngBlock + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kDngBlock) {
    DngG g = {};
    if (demodulate) g = dng_guide(guides[2 * i], guides[2 * i + 1]);
    const DnPx p = dng_store_px(dng_from4(img[i]), g, demodulate);
    float* o = out_rgb + 3 * i;
    o[0] = p.r;
    o[1] = p.g;
    o[2] = p.b;
    if (out_var) out_var[i] = p.v;
  }
}

// One block per 16 x 16 tile, tiles in row-major order over a 1-D grid, as dn_pass.
template <bool STEP_SMALL>
__global__ __launch_bounds__(kDngBlock) void dng_pass(const float4* __restrict__ in, const float4* __restrict__ guides,
                                                      float4* __restrict__ out, int32_t width, int32_t height,
                                                      int32_t tiles_x, int32_t step, DngParams prm) {
  const int32_t ty = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tx = (int32_t)(blockIdx.x - (uint32_t)ty * tiles_x);
  const int32_t x0 = tx * kDngTile, y0 = ty * kDngTile;
  const int32_t x = x0 + (int32_t)(threadIdx.x & (kDngTile - 1)), y = y0 + (int32_t)(threadIdx.x / kDngTile);
  const bool inside = x < width && y < height;
  auto guide = [&](int32_t qx, int32_t qy) {
    const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
    return dng_guide(guides[2 * q], guides[2 * q + 1]);
  };
  if (STEP_SMALL) {
    __shared__ float4 tile[kDngLdsRows * kDngLdsStride];
    const int32_t halo = 2 * step, side = kDngTile + 2 * halo;  // side <= kDngLdsRows <= kDngLdsStride
    for (int32_t i = (int32_t)threadIdx.x; i < side * side; i += kDngBlock) {
      const int32_t r = i / side, c = i - r * side;
      const int32_t gx = x0 - halo + c, gy = y0 - halo + r;
      if (gx >= 0 && gx < width && gy >= 0 && gy < height)  // cells outside the image are never read
        tile[r * kDngLdsStride + c] = in[(size_t)gy * (size_t)width + (size_t)gx];
    }
    __syncthreads();
    if (!inside) return;
    const DnPx o = dng_pass_px(
        x, y, width, height, step, prm,
        [&](int32_t qx, int32_t qy) {
          return dng_from4(tile[(qy - y0 + halo) * kDngLdsStride + (qx - x0 + halo)]);
        },
        guide);
    out[(size_t)y * (size_t)width + (size_t)x] = make_float4(o.r, o.g, o.b, o.v);
  } else {
    if (!inside) return;
    const DnPx o = dng_pass_px(
        x, y, width, height, step, prm,
        [&](int32_t qx, int32_t qy) { return dng_from4(in[(size_t)qy * (size_t)width + (size_t)qx]); }, guide);
    out[(size_t)y * (size_t)width + (size_t)x] = make_float4(o.r, o.g, o.b, o.v);
  }
}

// Which passes stage their colour taps in LDS: steps up to this one (0: none).
// Steps 1 and 2 by default; the setter exists for the A/B record of profiles/guided.
static int32_t g_lds_max_step = 2;

static hipError_t launch_denoise_guided(const float* accum, const float* stats, const float* guides, int32_t width,
                                        int32_t height, int32_t iterations, const DngParams& prm, void* ws,
                                        float* out_rgb, float* out_var, hipStream_t stream) {
  const int64_t npix = (int64_t)width * height;
  float4* buf[2] = {(float4*)ws, (float4*)ws + npix};
  const float4* g4 = (const float4*)guides;
  const int64_t nb = (npix + kDngBlock - 1) / kDngBlock;
  const dim3 flat((unsigned)(nb > 4096 ? 4096 : nb)), block(kDngBlock);
  hipLaunchKernelGGL(dng_load, flat, block, 0, stream, accum, (const float4*)stats, g4, buf[0], npix, prm.demodulate);
  const int32_t tiles_x = (width + kDngTile - 1) / kDngTile;
  const dim3 tiles((unsigned)((int64_t)tiles_x * ((height + kDngTile - 1) / kDngTile)));  // <= 2^31-1 pixels / 16 + rows
  int cur = 0;
  for (int32_t i = 0; i < iterations; ++i) {
    const int32_t step = 1 << i;
    if (step <= g_lds_max_step)
      hipLaunchKernelGGL(dng_pass<true>, tiles, block, 0, stream, buf[cur], g4, buf[cur ^ 1], width, height, tiles_x,
                         step, prm);
    else
      hipLaunchKernelGGL(dng_pass<false>, tiles, block, 0, stream, buf[cur], g4, buf[cur ^ 1], width, height, tiles_x,
                         step, prm);
    cur ^= 1;
  }
  hipLaunchKernelGGL(dng_store, flat, block, 0, stream, buf[cur], g4, out_rgb, out_var, npix, prm.demodulate);
  return hipGetLastError();
}

}  // namespace ptmi

using namespace ptmi;

static int64_t dng_pixels(int32_t width, int32_t height) {
  if (width < 1 || height < 1) return 0;
  const int64_t n = (int64_t)width * (int64_t)height;
  return n > 0x7fffffff ? 0 : n;
}

static bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

static int hip_result(hipError_t e) {
  if (e == hipSuccess) return PTMI_OK;
  set_last_error(PTMI_EHIP, hipGetErrorString(e));
  return PTMI_EHIP;
}

extern "C" {

int ptmi_guide_trace(const ptmi_scene_view* scene, const ptmi_frame* frame, float* guides, void* stream) {
  DevScene sc;
  DevFrame fr;
  int32_t slots = 0;
  if (int rc = guide_to_dev(scene, frame, sc, fr, slots)) return rc;
  if (!guides || ((uintptr_t)guides & 15u)) return set_last_error(PTMI_EINVAL, "guide_trace: guides NULL/misaligned");
  if (fr.x0 != 0 || fr.y0 != 0 || fr.w != fr.width || fr.h != fr.height)
    return set_last_error(PTMI_EINVAL, "guide_trace: the frame is windowed (guides are whole-frame)");
  if (fr.band_stride != 1) return set_last_error(PTMI_EINVAL, "guide_trace: the frame is banded (guides are whole-frame)");
  return hip_result(launch_guide_trace(sc, fr, slots, guides, (hipStream_t)stream));
}

int ptmi_denoise_guided(const float* accum, const float* stats, const float* guides, int32_t width, int32_t height,
                        const ptmi_dn_guided_params* params, void* workspace, size_t workspace_bytes, float* out_rgb,
                        float* out_var, void* stream) {
  if (!accum) return set_last_error(PTMI_EINVAL, "denoise_guided: accum is NULL");
  if (!stats || ((uintptr_t)stats & 15u)) return set_last_error(PTMI_EINVAL, "denoise_guided: stats NULL/misaligned");
  if (!guides || ((uintptr_t)guides & 15u))
    return set_last_error(PTMI_EINVAL, "denoise_guided: guides NULL/misaligned");
  if (!params) return set_last_error(PTMI_EINVAL, "denoise_guided: params is NULL");
  if (!workspace || ((uintptr_t)workspace & 15u))
    return set_last_error(PTMI_EINVAL, "denoise_guided: workspace NULL/misaligned");
  if (!out_rgb) return set_last_error(PTMI_EINVAL, "denoise_guided: out_rgb is NULL");
  const int64_t npix = dng_pixels(width, height);
  if (npix == 0)
    return set_last_error(PTMI_EINVAL,
                          "denoise_guided: bad image size (width and height >= 1, at most 2^31-1 pixels)");
  if (params->iterations < 0 || params->iterations > kDnMaxIterations)
    return set_last_error(PTMI_EINVAL, "denoise_guided: iterations must be in [0, 8]");
  if (!(params->sigma >= 0.0f)) return set_last_error(PTMI_EINVAL, "denoise_guided: sigma must be >= 0");
  if (!(params->sigma_z >= 0.0f)) return set_last_error(PTMI_EINVAL, "denoise_guided: sigma_z must be >= 0");
  if (!(params->sigma_a >= 0.0f)) return set_last_error(PTMI_EINVAL, "denoise_guided: sigma_a must be >= 0");
  if (params->normal_power_log2 < 0 || params->normal_power_log2 > kDngMaxNormalPower)
    return set_last_error(PTMI_EINVAL, "denoise_guided: normal_power_log2 must be in [0, 7]");
  if (params->flags & ~PTMI_DN_DEMODULATE) return set_last_error(PTMI_EINVAL, "denoise_guided: unknown flag bits");
  if (workspace_bytes < dn_workspace_bytes(npix))
    return set_last_error(PTMI_EINVAL, "denoise_guided: workspace too small");
  const uint64_t n = (uint64_t)npix;
  if (overlap(out_rgb, 12 * n, accum, 12 * n)) return set_last_error(PTMI_EINVAL, "denoise_guided: out_rgb aliases accum");
  if (overlap(out_rgb, 12 * n, stats, 16 * n)) return set_last_error(PTMI_EINVAL, "denoise_guided: out_rgb aliases stats");
  if (overlap(out_rgb, 12 * n, guides, 32 * n))
    return set_last_error(PTMI_EINVAL, "denoise_guided: guides aliases out_rgb");
  if (out_var && overlap(out_var, 4 * n, guides, 32 * n))
    return set_last_error(PTMI_EINVAL, "denoise_guided: guides aliases out_var");
  DngParams prm;
  prm.sigma = params->sigma;
  prm.sigma_z = params->sigma_z;
  prm.sigma_a = params->sigma_a;
  prm.normal_power_log2 = params->normal_power_log2;
  prm.demodulate = (params->flags & PTMI_DN_DEMODULATE) ? 1 : 0;
  return hip_result(launch_denoise_guided(accum, stats, guides, width, height, params->iterations, prm, workspace,
                                          out_rgb, out_var, (hipStream_t)stream));
}

int ptmi_denoise_guided_set_lds_max_step(int32_t max_step) {
  if (max_step < 0 || max_step > 2)
    return set_last_error(PTMI_EINVAL, "denoise_guided: the LDS form covers steps 1 and 2");
  const int32_t prev = g_lds_max_step;
  g_lds_max_step = max_step;
  return prev;
}

}  // extern "C"
