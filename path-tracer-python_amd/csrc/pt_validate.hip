// pt_validate.hip — the history-validation ABI (include/ptmi_validate.h): a
// carried history compared with a few fresh samples over a window, the stale
// part dropped, the two merged.
//
//   * vd_validate: one 256-lane block per 16 x 16 pixel tile (pt_image.hpp).
//     The block first stages step 1 ({d, v, usable}) of its tile and the
//     `radius` halo around it in LDS: (16 + 2 radius)^2 entries, at most
//     30 x 30, each lane computing entries tid, tid + 256, ... from the two
//     16-B stats loads of the entry's pixel. Entries outside the image are
//     zeros, and every lane of the block, inside the frame or not, reaches the
//     one __syncthreads(). Then each lane inside the frame sums its window from
//     LDS in the contract's order and does steps 3 - 6 from its own pixel's
//     loads: two 16-B stats loads and two accum pixels of three dwords. One
//     16-B store, three dwords and, if asked for, the weight per pixel. No
//     cross-lane register reads.
//
//     LDS layout: {d, v} as one float2 array (one ds_read_b64 per window
//     pixel) and `usable` as a dword array, both with a row pitch of 48
//     entries whatever the radius. A wave is a 16 x 4 pixel strip and a
//     32-lane bank group two rows of it; with a pitch of 16 mod 32 the two
//     rows of a group fall on disjoint banks for the 8-B reads (64 banks) and
//     the 4-B reads (32 banks) alike. 30 rows x 48 x 12 B = 17280 B per block:
//     nine blocks a CU by LDS, more than the eight that 32 waves allow.
//
// The arithmetic is pt_validate_math.hpp's, shared with validate_check.cpp; the
// kernel only decides where a value is read from. No render kernel is
// involved. Not timed by ptmi_prof_*.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_validate.h"
#include "pt_args.hpp"
#include "pt_image.hpp"
#include "pt_validate_math.hpp"

namespace ptmi {

constexpr int kVdSideMax = kImgTile + 2 * kVdMaxRadius;  // 30
constexpr int kVdPitch = 48;                             // >= kVdSideMax, 16 mod 32
static_assert(kVdPitch >= kVdSideMax && kVdPitch % 32 == 16, "the LDS row pitch");

__global__ __launch_bounds__(kImgBlock) void vd_validate(const float* __restrict__ hist_accum,
                                                        const float4* __restrict__ hist_stats,
                                                        const float* __restrict__ fresh_accum,
                                                        const float4* __restrict__ fresh_stats, VdParams prm,
                                                        float* __restrict__ out_accum, float4* __restrict__ out_stats,
                                                        float* __restrict__ weight_out, int32_t width, int32_t height,
                                                        int32_t tiles_x) {
  __shared__ float2 s_dv[kVdSideMax * kVdPitch];
  __shared__ uint32_t s_usable[kVdSideMax * kVdPitch];
  const TileXY t = tile_xy<kImgTile>(tiles_x);
  const int32_t radius = prm.radius;
  const int32_t side = kImgTile + 2 * radius;
  const int32_t hx0 = t.x0 - radius, hy0 = t.y0 - radius;  // the halo's origin (may lie outside the image)
  auto index = [&](int32_t qx, int32_t qy) { return (size_t)qy * (size_t)width + (size_t)qx; };

  for (int32_t e = (int32_t)threadIdx.x; e < side * side; e += kImgBlock) {
    const int32_t ey = e / side, ex = e - ey * side;
    const int32_t qx = hx0 + ex, qy = hy0 + ey;
    VdEntry en = {0.0f, 0.0f, 0u};
    if (qx >= 0 && qx < width && qy >= 0 && qy < height) {
      const float4 h = hist_stats[index(qx, qy)], f = fresh_stats[index(qx, qy)];
      en = vd_entry(RpStats{h.x, h.y, h.z, h.w}, RpStats{f.x, f.y, f.z, f.w});
    }
    s_dv[ey * kVdPitch + ex] = make_float2(en.d, en.v);
    s_usable[ey * kVdPitch + ex] = en.usable;
  }
  __syncthreads();  // reached by every lane: nothing above returns
  const int32_t x = t.x, y = t.y;
  if (x >= width || y >= height) return;

  const VdSum sum = vd_window(x, y, width, height, radius, [&](int32_t qx, int32_t qy) {
    const int32_t at = (qy - hy0) * kVdPitch + (qx - hx0);  // inside the halo: |qx - x|, |qy - y| <= radius
    const float2 dv = s_dv[at];
    return VdEntry{dv.x, dv.y, s_usable[at]};
  });
  const float lam = vd_lambda(sum, prm.k_lo, prm.k_hi);

  const size_t p = index(x, y);
  const float4 hs = hist_stats[p], fs = fresh_stats[p];
  const float *ha = hist_accum + 3 * p, *fa = fresh_accum + 3 * p;
  const VdOut o = vd_merge(RpRgb{ha[0], ha[1], ha[2]}, RpStats{hs.x, hs.y, hs.z, hs.w}, RpRgb{fa[0], fa[1], fa[2]},
                           RpStats{fs.x, fs.y, fs.z, fs.w}, lam);
  out_stats[p] = make_float4(o.stats.n, o.stats.mean, o.stats.m2, o.stats.pad);
  float* a = out_accum + 3 * p;
  a[0] = o.accum.r;
  a[1] = o.accum.g;
  a[2] = o.accum.b;
  if (weight_out) weight_out[p] = o.weight;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_history_validate(const float* hist_accum, const float* hist_stats, const float* fresh_accum,
                          const float* fresh_stats, int32_t width, int32_t height, const ptmi_validate_params* params,
                          float* out_accum, float* out_stats, float* weight_out, void* stream) {
  const char* what = "history_validate";
  if (bad4(hist_accum)) return fail(PTMI_EINVAL, "%s: hist_accum NULL/misaligned", what);
  if (bad16(hist_stats)) return fail(PTMI_EINVAL, "%s: hist_stats NULL/misaligned", what);
  if (bad4(fresh_accum)) return fail(PTMI_EINVAL, "%s: fresh_accum NULL/misaligned", what);
  if (bad16(fresh_stats)) return fail(PTMI_EINVAL, "%s: fresh_stats NULL/misaligned", what);
  if (!params) return fail(PTMI_EINVAL, "%s: params is NULL", what);
  if (bad4(out_accum)) return fail(PTMI_EINVAL, "%s: out_accum NULL/misaligned", what);
  if (bad16(out_stats)) return fail(PTMI_EINVAL, "%s: out_stats NULL/misaligned", what);
  if (weight_out && bad4(weight_out)) return fail(PTMI_EINVAL, "%s: weight_out misaligned", what);
  const uint64_t n = (uint64_t)image_pixels(width, height);
  if (n == 0) return fail(PTMI_EINVAL, "%s: bad image size (width and height >= 1, at most 2^31-1 pixels)", what);
  if (params->radius < 0 || params->radius > PTMI_VALIDATE_MAX_RADIUS)
    return fail(PTMI_EINVAL, "%s: radius must be in [0, %d]", what, PTMI_VALIDATE_MAX_RADIUS);
  if (!(dn_finite(params->k_lo) && dn_finite(params->k_hi)))
    return fail(PTMI_EINVAL, "%s: k_lo and k_hi must be finite", what);
  if (!(params->k_lo >= 0.0f)) return fail(PTMI_EINVAL, "%s: k_lo must be >= 0", what);
  if (!(params->k_hi > params->k_lo)) return fail(PTMI_EINVAL, "%s: k_hi must be above k_lo", what);
  const struct {
    const char* name;
    const void* p;
    uint64_t bytes;
  } in[4] = {{"hist_accum", hist_accum, 12 * n},
             {"hist_stats", hist_stats, 16 * n},
             {"fresh_accum", fresh_accum, 12 * n},
             {"fresh_stats", fresh_stats, 16 * n}},
    out[3] = {{"out_accum", out_accum, 12 * n}, {"out_stats", out_stats, 16 * n}, {"weight_out", weight_out, 4 * n}};
  for (int o = 0; o < 3; ++o) {
    if (!out[o].p) continue;  // no weight image
    for (const auto& i : in)
      if (overlaps(out[o].p, out[o].bytes, i.p, i.bytes))
        return fail(PTMI_EINVAL, "%s: %s aliases %s", what, out[o].name, i.name);
    for (int k = 0; k < o; ++k)
      if (overlaps(out[o].p, out[o].bytes, out[k].p, out[k].bytes))
        return fail(PTMI_EINVAL, "%s: %s aliases %s", what, out[o].name, out[k].name);
  }
  const VdParams prm = {params->radius, params->k_lo, params->k_hi};
  hipLaunchKernelGGL(vd_validate, image_tile_grid(width, height, kImgTile), dim3(kImgBlock), 0, (hipStream_t)stream,
                     hist_accum, (const float4*)hist_stats, fresh_accum, (const float4*)fresh_stats, prm, out_accum,
                     (float4*)out_stats, weight_out, width, height, image_tiles_x(width, kImgTile));
  return hip_result(hipGetLastError());
}

}  // extern "C"
