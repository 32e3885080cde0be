// reproject_check.cpp — the temporal reprojection's per-pixel arithmetic
// (pt_reproject_math.hpp, the function the kernel of pt_reproject.hip calls)
// run on the CPU: a stand-alone host program, no HIP, no GPU. `make
// reproject_check` builds it; tests/test_reproject_check.py compares its output
// with the numpy reference bit for bit.
//
//   reproject_check WIDTH HEIGHT in.f32 accum_out.f32 stats_out.f32
//
// in.f32 is raw little-endian f32: the current camera and the previous camera
// (center, pixel00, delta_u, delta_v: 12 values each), the parameters
// (max_history, sigma_z, normal_min, sigma_a), then guides_cur (H x W x 8),
// guides_prev (H x W x 8), accum_prev (H x W x 3) and stats_prev (H x W x 4).
// Writes raw accum_out (H x W x 3) and stats_out (H x W x 4). Exit 0 on
// success, 2 on bad arguments or I/O.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pt_check_io.hpp"
#include "pt_reproject_math.hpp"

using namespace ptmi;

static RpCam camera(const float* s) {
  RpCam c;
  for (int k = 0; k < 3; ++k) {
    c.center[k] = s[k];
    c.pixel00[k] = s[3 + k];
    c.delta_u[k] = s[6 + k];
    c.delta_v[k] = s[9 + k];
  }
  return c;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s WIDTH HEIGHT in.f32 accum_out.f32 stats_out.f32\n", argv[0]);
    return 2;
  }
  const int32_t width = atoi(argv[1]), height = atoi(argv[2]);
  if (width < 1 || height < 1 || (int64_t)width * height > (1 << 26)) {
    fprintf(stderr, "bad size\n");
    return 2;
  }
  const size_t npix = (size_t)width * (size_t)height, head = 12 + 12 + 4;
  std::vector<float> in(head + (8 + 8 + 3 + 4) * npix);
  if (!read_f32(argv[3], in)) {
    fprintf(stderr, "cannot read two cameras, the parameters and %zu pixels of four images\n", npix);
    return 2;
  }
  const RpCam cur = camera(in.data()), prev = camera(in.data() + 12);
  const RpParams prm = {in[24], in[25], in[26], in[27]};
  if (!(prm.max_history >= 1.0f && prm.max_history <= kRpMaxHistory) || !(prm.sigma_z >= 0.0f) ||
      !(prm.normal_min >= -1.0f && prm.normal_min <= 1.0f) || !(prm.sigma_a >= 0.0f)) {
    fprintf(stderr, "bad parameters\n");
    return 2;
  }
  const float* gc = in.data() + head;
  const float* gp = gc + 8 * npix;
  const float* ap = gp + 8 * npix;
  const float* sp = ap + 3 * npix;
  auto guide = [&](const float* g, int32_t x, int32_t y) {
    const float* s = g + 8 * ((size_t)y * width + x);
    return DngG{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
  };
  std::vector<float> accum(3 * npix), stats(4 * npix);
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) {
      const RpOut o = rp_reproject_px(
          x, y, width, height, cur, prev, prm, [&](int32_t qx, int32_t qy) { return guide(gc, qx, qy); },
          [&](int32_t qx, int32_t qy) { return guide(gp, qx, qy); },
          [&](int32_t qx, int32_t qy) {
            const float* a = ap + 3 * ((size_t)qy * width + qx);
            return RpRgb{a[0], a[1], a[2]};
          },
          [&](int32_t qx, int32_t qy) {
            const float* s = sp + 4 * ((size_t)qy * width + qx);
            return RpStats{s[0], s[1], s[2], s[3]};
          });
      const size_t p = (size_t)y * width + x;
      accum[3 * p] = o.accum.r;
      accum[3 * p + 1] = o.accum.g;
      accum[3 * p + 2] = o.accum.b;
      stats[4 * p] = o.stats.n;
      stats[4 * p + 1] = o.stats.mean;
      stats[4 * p + 2] = o.stats.m2;
      stats[4 * p + 3] = o.stats.pad;
    }
  if (!write_f32(argv[4], accum) || !write_f32(argv[5], stats)) {
    fprintf(stderr, "cannot write the outputs\n");
    return 2;
  }
  return 0;
}
