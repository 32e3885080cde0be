// pt_reproject.hip — the temporal ABI (include/ptmi_temporal.h): reprojection
// of a stats render's history to a new camera.
//
//   * rp_reproject: one lane per pixel of the current frame, one block per
//     16 x 16 pixel tile, so a wave is a 16 x 4 pixel strip and the four
//     bilinear taps of neighbouring lanes fall on neighbouring pixels of the
//     previous frame: the gather is served by the caches. The centre's guide
//     pixel is two 16-B loads; a tap's stats pixel is one 16-B load, its guide
//     pixel two, and its accum pixel three dwords (12-B pixels are not 16-B
//     aligned). One 16-B store and three dwords per pixel. No cross-lane reads,
//     no LDS.
//
// The arithmetic is pt_reproject_math.hpp's, shared with reproject_check.cpp;
// the kernel only decides where a pixel is read from. No render kernel, no
// denoise kernel and no guide kernel is involved. Not timed by ptmi_prof_*.
#include <hip/hip_runtime.h>

#include "../../include/ptmi.h"
#include "../../include/ptmi_temporal.h"
#include "pt_reproject_math.hpp"

namespace ptmi {

int set_last_error(int code, const char* msg);  // pt_abi.hip: the text of ptmi_last_error()

constexpr int kRpTile = 16;  // a block is 16 x 16 pixels
constexpr int kRpBlock = kRpTile * kRpTile;

// One block per tile, tiles in row-major order over a 1-D grid, as dn_pass.
__global__ __launch_bounds__(kRpBlock) void rp_reproject(RpCam cur, RpCam prev, RpParams prm,
                                                         const float4* __restrict__ guides_cur,
                                                         const float4* __restrict__ guides_prev,
                                                         const float* __restrict__ accum_prev,
                                                         const float4* __restrict__ stats_prev,
                                                         float* __restrict__ accum_out, float4* __restrict__ stats_out,
                                                         int32_t width, int32_t height, int32_t tiles_x) {
  const int32_t ty = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tx = (int32_t)(blockIdx.x - (uint32_t)ty * tiles_x);
  const int32_t x = tx * kRpTile + (int32_t)(threadIdx.x & (kRpTile - 1)), y = ty * kRpTile + (int32_t)(threadIdx.x / kRpTile);
  if (x >= width || y >= height) return;
  auto index = [&](int32_t qx, int32_t qy) { return (size_t)qy * (size_t)width + (size_t)qx; };
  auto guide_of = [&](const float4* __restrict__ guides, size_t q) {
    const float4 n = guides[2 * q], a = guides[2 * q + 1];
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
  };
  const RpOut o = rp_reproject_px(
      x, y, width, height, cur, prev, prm, [&](int32_t qx, int32_t qy) { return guide_of(guides_cur, index(qx, qy)); },
      [&](int32_t qx, int32_t qy) { return guide_of(guides_prev, index(qx, qy)); },
      [&](int32_t qx, int32_t qy) {
        const float* a = accum_prev + 3 * index(qx, qy);
        return RpRgb{a[0], a[1], a[2]};
      },
      [&](int32_t qx, int32_t qy) {
        const float4 s = stats_prev[index(qx, qy)];
        return RpStats{s.x, s.y, s.z, s.w};
      });
  const size_t p = index(x, y);
  stats_out[p] = make_float4(o.stats.n, o.stats.mean, o.stats.m2, o.stats.pad);
  float* a = accum_out + 3 * p;
  a[0] = o.accum.r;
  a[1] = o.accum.g;
  a[2] = o.accum.b;
}

static RpCam rp_cam(const ptmi_camera* c) {
  RpCam r;
  for (int k = 0; k < 3; ++k) {
    r.center[k] = c->center[k];
    r.pixel00[k] = c->pixel00[k];
    r.delta_u[k] = c->delta_u[k];
    r.delta_v[k] = c->delta_v[k];
  }
  return r;
}

static hipError_t launch_reproject(const RpCam& cur, const RpCam& prev, const RpParams& prm, const float* guides_cur,
                                   const float* guides_prev, const float* accum_prev, const float* stats_prev,
                                   int32_t width, int32_t height, float* accum_out, float* stats_out,
                                   hipStream_t stream) {
  const int32_t tiles_x = (width + kRpTile - 1) / kRpTile;
  const dim3 tiles((unsigned)((int64_t)tiles_x * ((height + kRpTile - 1) / kRpTile)));  // <= 2^31-1 pixels / 16 + rows
  hipLaunchKernelGGL(rp_reproject, tiles, dim3(kRpBlock), 0, stream, cur, prev, prm, (const float4*)guides_cur,
                     (const float4*)guides_prev, accum_prev, (const float4*)stats_prev, accum_out, (float4*)stats_out,
                     width, height, tiles_x);
  return hipGetLastError();
}

}  // namespace ptmi

using namespace ptmi;

static bool rp_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

extern "C" {

int ptmi_reproject(const ptmi_camera* cur, const ptmi_camera* prev, const float* guides_cur, const float* guides_prev,
                   const float* accum_prev, const float* stats_prev, int32_t width, int32_t height,
                   const ptmi_reproject_params* params, float* accum_out, float* stats_out, void* stream) {
  if (!cur || !prev) return set_last_error(PTMI_EINVAL, "reproject: a camera is NULL");
  if (!guides_cur || ((uintptr_t)guides_cur & 15u))
    return set_last_error(PTMI_EINVAL, "reproject: guides_cur NULL/misaligned");
  if (!guides_prev || ((uintptr_t)guides_prev & 15u))
    return set_last_error(PTMI_EINVAL, "reproject: guides_prev NULL/misaligned");
  if (!accum_prev) return set_last_error(PTMI_EINVAL, "reproject: accum_prev is NULL");
  if (!stats_prev || ((uintptr_t)stats_prev & 15u))
    return set_last_error(PTMI_EINVAL, "reproject: stats_prev NULL/misaligned");
  if (!params) return set_last_error(PTMI_EINVAL, "reproject: params is NULL");
  if (!accum_out) return set_last_error(PTMI_EINVAL, "reproject: accum_out is NULL");
  if (!stats_out || ((uintptr_t)stats_out & 15u))
    return set_last_error(PTMI_EINVAL, "reproject: stats_out NULL/misaligned");
  if (width < 1 || height < 1 || (int64_t)width * (int64_t)height > 0x7fffffff)
    return set_last_error(PTMI_EINVAL, "reproject: bad image size (width and height >= 1, at most 2^31-1 pixels)");
  const uint64_t n = (uint64_t)width * (uint64_t)height;
  const struct {
    const void* p;
    uint64_t bytes;
    const char* msg_accum;
    const char* msg_stats;
  } in[4] = {{guides_cur, 32 * n, "reproject: accum_out aliases guides_cur", "reproject: stats_out aliases guides_cur"},
             {guides_prev, 32 * n, "reproject: accum_out aliases guides_prev", "reproject: stats_out aliases guides_prev"},
             {accum_prev, 12 * n, "reproject: accum_out aliases accum_prev", "reproject: stats_out aliases accum_prev"},
             {stats_prev, 16 * n, "reproject: accum_out aliases stats_prev", "reproject: stats_out aliases stats_prev"}};
  for (const auto& i : in) {
    if (rp_overlap(accum_out, 12 * n, i.p, i.bytes)) return set_last_error(PTMI_EINVAL, i.msg_accum);
    if (rp_overlap(stats_out, 16 * n, i.p, i.bytes)) return set_last_error(PTMI_EINVAL, i.msg_stats);
  }
  if (rp_overlap(accum_out, 12 * n, stats_out, 16 * n))
    return set_last_error(PTMI_EINVAL, "reproject: accum_out aliases stats_out");
  if (!(params->max_history >= 1.0f && params->max_history <= kRpMaxHistory))
    return set_last_error(PTMI_EINVAL, "reproject: max_history must be in [1, 2^24]");
  if (!(params->sigma_z >= 0.0f)) return set_last_error(PTMI_EINVAL, "reproject: sigma_z must be >= 0");
  if (!(params->normal_min >= -1.0f && params->normal_min <= 1.0f))
    return set_last_error(PTMI_EINVAL, "reproject: normal_min must be in [-1, 1]");
  if (!(params->sigma_a >= 0.0f)) return set_last_error(PTMI_EINVAL, "reproject: sigma_a must be >= 0");
  if (params->flags != 0) return set_last_error(PTMI_EINVAL, "reproject: flags must be 0");
  RpParams prm;
  prm.max_history = params->max_history;
  prm.sigma_z = params->sigma_z;
  prm.normal_min = params->normal_min;
  prm.sigma_a = params->sigma_a;
  const hipError_t e = launch_reproject(rp_cam(cur), rp_cam(prev), prm, guides_cur, guides_prev, accum_prev, stats_prev,
                                        width, height, accum_out, stats_out, (hipStream_t)stream);
  if (e == hipSuccess) return PTMI_OK;
  return set_last_error(PTMI_EHIP, hipGetErrorString(e));
}

}  // extern "C"
