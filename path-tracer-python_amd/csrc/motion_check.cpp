// motion_check.cpp — the motion-aware reprojection's per-pixel arithmetic
// (pt_motion_math.hpp and pt_reproject_math.hpp, the functions the kernel of
// pt_motion.hip calls) run on the CPU: a stand-alone host program, no HIP, no
// GPU. `make motion_check` builds it; tests/test_motion_abi.py compares its
// output with the numpy reference bit for bit.
//
//   motion_check WIDTH HEIGHT NS NQ NT FLAGS in.f32 ids.i32 accum_out.f32 stats_out.f32
//
// in.f32 is raw little-endian f32: the current camera and the previous camera
// (center, pixel00, delta_u, delta_v: 12 values each), the parameters
// (max_history, sigma_z, normal_min, sigma_a), guides_cur (H x W x 8),
// guides_prev (H x W x 8), accum_prev (H x W x 3), stats_prev (H x W x 4), then
// the current rows (NS x 4 spheres, NQ x 16 quads, NT x 12 triangles) and the
// previous rows in the same order. ids.i32 is raw i32: ids_cur, then ids_prev
// (H x W each). FLAGS: PTMI_RPM_* (bit 0: match the ids). Writes raw accum_out
// (H x W x 3) and stats_out (H x W x 4). Exit 0 on success, 2 on bad arguments
// or I/O.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pt_check_io.hpp"
#include "pt_motion_math.hpp"

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

template <int N>
static void row(const float* rows, int32_t prim, float (&out)[N]) {
  for (int k = 0; k < N; ++k) out[k] = rows[(size_t)prim * N + k];
}

int main(int argc, char** argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s WIDTH HEIGHT NS NQ NT FLAGS in.f32 ids.i32 accum_out.f32 stats_out.f32\n", argv[0]);
    return 2;
  }
  const int32_t width = atoi(argv[1]), height = atoi(argv[2]);
  const MvCounts counts = {atoi(argv[3]), atoi(argv[4]), atoi(argv[5])};
  const int32_t flags = atoi(argv[6]);
  if (width < 1 || height < 1 || (int64_t)width * height > (1 << 26) || counts.spheres < 0 || counts.quads < 0 ||
      counts.tris < 0 || counts.spheres > (1 << 20) || counts.quads > (1 << 20) || counts.tris > (1 << 20) ||
      (flags & ~1)) {
    fprintf(stderr, "bad size, counts or flags\n");
    return 2;
  }
  const size_t npix = (size_t)width * (size_t)height, head = 12 + 12 + 4;
  const size_t nrows = (size_t)kMvSphereFloats * counts.spheres + (size_t)kMvQuadFloats * counts.quads +
                       (size_t)kMvTriFloats * counts.tris;
  std::vector<float> in(head + (8 + 8 + 3 + 4) * npix + 2 * nrows);
  std::vector<int32_t> ids(2 * npix);
  if (!read_f32(argv[7], in) || !read_i32(argv[8], ids)) {
    fprintf(stderr, "cannot read two cameras, the parameters, %zu pixels of four images, %zu row values twice and "
                    "two id images\n", npix, nrows);
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
  const float* rows[2][3];  // [current, previous][spheres, quads, tris]
  const float* at = sp + 4 * npix;
  for (int which = 0; which < 2; ++which) {
    rows[which][0] = at;
    rows[which][1] = rows[which][0] + (size_t)kMvSphereFloats * counts.spheres;
    rows[which][2] = rows[which][1] + (size_t)kMvQuadFloats * counts.quads;
    at = rows[which][2] + (size_t)kMvTriFloats * counts.tris;
  }
  const int32_t* ic = ids.data();
  const int32_t* ip = ic + npix;
  auto guide = [&](const float* g, int32_t x, int32_t y) {
    const float* s = g + 8 * ((size_t)y * width + x);
    return DngG{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
  };
  std::vector<float> accum(3 * npix), stats(4 * npix);
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) {
      const RpOut o = mv_reproject_px(
          x, y, width, height, cur, prev, prm, (flags & 1) != 0, counts,
          [&](int32_t qx, int32_t qy) { return guide(gc, qx, qy); },
          [&](int32_t qx, int32_t qy) { return ic[(size_t)qy * width + qx]; },
          [&](RpV3 P, const MvId& m) {
            if (m.type == kMvSphere) {
              float a[kMvSphereFloats], b[kMvSphereFloats];
              row(rows[0][0], m.prim, a);
              row(rows[1][0], m.prim, b);
              return mv_sphere_prev(P, a, b);
            }
            if (m.type == kMvQuad) {
              float a[kMvQuadFloats], b[kMvQuadFloats];
              row(rows[0][1], m.prim, a);
              row(rows[1][1], m.prim, b);
              return mv_quad_prev(P, a, b);
            }
            float a[kMvTriFloats], b[kMvTriFloats];
            row(rows[0][2], m.prim, a);
            row(rows[1][2], m.prim, b);
            return mv_tri_prev(P, a, b);
          },
          [&](int32_t qx, int32_t qy) { return guide(gp, qx, qy); },
          [&](int32_t qx, int32_t qy) {
            const float* a = ap + 3 * ((size_t)qy * width + qx);
            return RpRgb{a[0], a[1], a[2]};
          },
          [&](int32_t qx, int32_t qy) {
            const float* s = sp + 4 * ((size_t)qy * width + qx);
            return RpStats{s[0], s[1], s[2], s[3]};
          },
          [&](int32_t qx, int32_t qy) { return ip[(size_t)qy * width + qx]; });
      const size_t p = (size_t)y * width + x;
      accum[3 * p] = o.accum.r;
      accum[3 * p + 1] = o.accum.g;
      accum[3 * p + 2] = o.accum.b;
      stats[4 * p] = o.stats.n;
      stats[4 * p + 1] = o.stats.mean;
      stats[4 * p + 2] = o.stats.m2;
      stats[4 * p + 3] = o.stats.pad;
    }
  if (!write_f32(argv[9], accum) || !write_f32(argv[10], stats)) {
    fprintf(stderr, "cannot write the outputs\n");
    return 2;
  }
  return 0;
}
