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

#include "../../include/ptmi_temporal.h"
#include "pt_image.hpp"
#include "pt_reproject_args.hpp"

namespace ptmi {

// One block per 16 x 16 tile (pt_image.hpp), as dn_pass.
__global__ __launch_bounds__(kImgBlock) void rp_reproject(RpCam cur, RpCam prev, RpParams prm,
                                                         const float4* __restrict__ guides_cur,
                                                         const float4* __restrict__ guides_prev,
                                                         const float* __restrict__ accum_prev,
                                                         const float4* __restrict__ stats_prev,
                                                         float* __restrict__ accum_out, float4* __restrict__ stats_out,
                                                         int32_t width, int32_t height, int32_t tiles_x) {
  const TileXY t = tile_xy<kImgTile>(tiles_x);
  const int32_t x = t.x, y = t.y;
  if (x >= width || y >= height) return;
  auto index = [&](int32_t qx, int32_t qy) { return (size_t)qy * (size_t)width + (size_t)qx; };
  const RpOut o = rp_reproject_px(
      x, y, width, height, cur, prev, prm,
      [&](int32_t qx, int32_t qy) { return load_guide(guides_cur, index(qx, qy)); },
      [&](int32_t qx, int32_t qy) { return load_guide(guides_prev, index(qx, qy)); },
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

static hipError_t launch_reproject(const RpCam& cur, const RpCam& prev, const RpParams& prm, const float* guides_cur,
                                   const float* guides_prev, const float* accum_prev, const float* stats_prev,
                                   int32_t width, int32_t height, float* accum_out, float* stats_out,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(rp_reproject, image_tile_grid(width, height, kImgTile), dim3(kImgBlock), 0, stream, cur, prev,
                     prm, (const float4*)guides_cur, (const float4*)guides_prev, accum_prev, (const float4*)stats_prev,
                     accum_out, (float4*)stats_out, width, height, image_tiles_x(width, kImgTile));
  return hipGetLastError();
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_reproject(const ptmi_camera* cur, const ptmi_camera* prev, const float* guides_cur, const float* guides_prev,
                   const float* accum_prev, const float* stats_prev, int32_t width, int32_t height,
                   const ptmi_reproject_params* params, float* accum_out, float* stats_out, void* stream) {
  uint64_t n = 0;
  if (int rc = reproject_pointer_args("reproject", cur, prev, guides_cur, guides_prev, accum_prev, stats_prev, width,
                                      height, params, accum_out, stats_out, n))
    return rc;
  const RpBuffer in[4] = {{"guides_cur", guides_cur, 32 * n},
                          {"guides_prev", guides_prev, 32 * n},
                          {"accum_prev", accum_prev, 12 * n},
                          {"stats_prev", stats_prev, 16 * n}};
  if (int rc = reproject_overlap_args("reproject", in, 4, accum_out, stats_out, n)) return rc;
  RpParams prm;
  if (int rc = reproject_param_args("reproject", params, prm)) return rc;
  if (params->flags != 0) return fail(PTMI_EINVAL, "reproject: flags must be 0");
  return hip_result(launch_reproject(rp_cam(cur), rp_cam(prev), prm, guides_cur, guides_prev, accum_prev, stats_prev,
                                     width, height, accum_out, stats_out, (hipStream_t)stream));
}

}  // extern "C"
