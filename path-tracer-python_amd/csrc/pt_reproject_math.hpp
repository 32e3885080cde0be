// pt_reproject_math.hpp — the per-pixel arithmetic of the temporal
// reprojection (include/ptmi_temporal.h states the contract), shared by the
// kernel of pt_reproject.hip and the CPU check program reproject_check.cpp.
// Steps 1, 2 and 3 - 7 are separate functions: the motion-aware reprojection
// (pt_motion_math.hpp) puts its own step 2' between them.
//
// Host/device, no HIP type. A guide pixel is pt_denoise_math.hpp's DngG, a stats
// pixel and an accum pixel are RpStats and RpRgb; the caller decides where they
// are read from. Every operation is f32 with one rounding, in the order written
// here, so numpy f32 reproduces every value bit for bit
// (tests/reproject_helpers.py).
#pragma once
#include "pt_denoise_math.hpp"

namespace ptmi {

struct RpCam {  // the four vectors of ptmi_camera the reprojection reads
  float center[3], pixel00[3], delta_u[3], delta_v[3];
};

struct RpParams {
  float max_history, sigma_z, normal_min, sigma_a;
};

struct RpRgb {
  float r, g, b;
};

struct alignas(16) RpStats {
  float n, mean, m2, pad;
};

struct RpOut {
  RpRgb accum;
  RpStats stats;
};

constexpr float kRpMaxHistory = 16777216.0f;  // 2^24: every integer up to it is an f32
constexpr float kRpDepthFloor = 1e-4f;

struct RpV3 {
  float x, y, z;
};

PTMI_DN_HD RpV3 rp_v3(const float* a) { return RpV3{a[0], a[1], a[2]}; }
PTMI_DN_HD RpV3 rp_sub(RpV3 a, RpV3 b) { return RpV3{a.x - b.x, a.y - b.y, a.z - b.z}; }
PTMI_DN_HD float rp_dot(RpV3 a, RpV3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
PTMI_DN_HD RpV3 rp_cross(RpV3 a, RpV3 b) {
  return RpV3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// Step 1: the primary ray of ptmi_guide_trace through pixel (px, py).
struct RpRay {
  RpV3 c, d;  // origin (the camera centre) and direction, not normalised
  float len;  // sqrtf(dot(d, d))
};

PTMI_DN_HD RpRay rp_primary_ray(int32_t px, int32_t py, const RpCam& cur) {
  const RpV3 c = rp_v3(cur.center), p00 = rp_v3(cur.pixel00), du = rp_v3(cur.delta_u), dv = rp_v3(cur.delta_v);
  const float fpx = (float)px, fpy = (float)py;
  const RpV3 ps = {(p00.x + du.x * fpx) + dv.x * fpy, (p00.y + du.y * fpx) + dv.y * fpy,
                   (p00.z + du.z * fpx) + dv.z * fpy};
  const RpV3 d = rp_sub(ps, c);
  return RpRay{c, d, sqrtf(rp_dot(d, d))};
}

// Step 2's surface point P of a hit pixel at guide depth `depth`.
PTMI_DN_HD RpV3 rp_surface_point(const RpRay& ray, float depth) {
  const float s = depth / ray.len;
  return RpV3{ray.c.x + ray.d.x * s, ray.c.y + ray.d.y * s, ray.c.z + ray.d.z * s};
}

// The tap predicate of a reprojection that has none.
struct RpEveryTap {
  PTMI_DN_HD bool operator()(int32_t, int32_t) const { return true; }
};

// Steps 3 - 7 for a current pixel whose guide pixel is g: v is step 2's vector
// from the previous camera (to the surface point for a hit, the ray direction
// for a miss), hit_p whether the pixel is a hit. guide_prev, accum_prev and
// stats_prev return the previous frame's pixels and are called only for
// coordinates inside the image: stats first, accum and guide only for a tap
// whose count is at least 2. tap_ok(qx, qy) is a further condition on the taps
// of a hit pixel (include/ptmi_motion.h's step 5'), asked before the tap's
// guide pixel is read.
template <class GuidePrev, class AccumPrev, class StatsPrev, class TapOk>
PTMI_DN_HD RpOut rp_history_px(RpV3 v, bool hit_p, const DngG& g, int32_t width, int32_t height, const RpCam& prev,
                               const RpParams& prm, GuidePrev&& guide_prev, AccumPrev&& accum_prev,
                               StatsPrev&& stats_prev, TapOk&& tap_ok) {
  RpOut out = {};  // a pixel without history: all zeros

  // 3. its pixel position (a, b) in the previous frame
  const RpV3 pdu = rp_v3(prev.delta_u), pdv = rp_v3(prev.delta_v);
  const RpV3 r = rp_sub(rp_v3(prev.pixel00), rp_v3(prev.center));
  const RpV3 w = rp_cross(pdu, pdv);
  const float lam = rp_dot(r, w) / rp_dot(v, w);
  const RpV3 q = {v.x * lam - r.x, v.y * lam - r.y, v.z * lam - r.z};
  const float a = rp_dot(q, pdu) / rp_dot(pdu, pdu);
  const float b = rp_dot(q, pdv) / rp_dot(pdv, pdv);
  const float zexp = sqrtf(rp_dot(v, v));

  // 4.
  if (!(lam > 0.0f && a > -1.0f && a < (float)width && b > -1.0f && b < (float)height)) return out;
  const float fx0 = floorf(a), fy0 = floorf(b);
  const float fx = a - fx0, fy = b - fy0;
  const int32_t x0 = (int32_t)fx0, y0 = (int32_t)fy0;  // -1 .. width - 1, -1 .. height - 1

  // 5., 6.
  const float tol_z = prm.sigma_z * zexp + kRpDepthFloor;
  float W = 0.0f, Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, S = 0.0f, N = 0.0f;
  for (int32_t j = 0; j < 2; ++j) {
    const int32_t qy = y0 + j;
    if (qy < 0 || qy >= height) continue;
    const float wy = j ? fy : 1.0f - fy;
    for (int32_t i = 0; i < 2; ++i) {
      const int32_t qx = x0 + i;
      if (qx < 0 || qx >= width) continue;
      const float wt = (i ? fx : 1.0f - fx) * wy;
      const RpStats st = stats_prev(qx, qy);
      if (!(st.n >= 2.0f)) continue;
      const RpRgb acc = accum_prev(qx, qy);
      const float scale = (float)(1.0 / (double)st.n);
      const float cr = acc.r * scale, cg = acc.g * scale, cb = acc.b * scale;
      const float s2 = st.m2 / (st.n - 1.0f);
      if (!(dn_finite(cr) && dn_finite(cg) && dn_finite(cb) && dn_finite(s2))) continue;
      if (hit_p && !tap_ok(qx, qy)) continue;
      const DngG gq = guide_prev(qx, qy);
      if ((gq.hit != 0.0f) != hit_p) continue;
      if (hit_p) {
        if (!(fabsf(gq.z - zexp) <= tol_z)) continue;
        if (!((g.nx * gq.nx + g.ny * gq.ny) + g.nz * gq.nz >= prm.normal_min)) continue;
        if (!((fabsf(g.ar - gq.ar) + fabsf(g.ag - gq.ag)) + fabsf(g.ab - gq.ab) <= prm.sigma_a)) continue;
      }
      W = W + wt;
      Cr = Cr + wt * cr;
      Cg = Cg + wt * cg;
      Cb = Cb + wt * cb;
      S = S + wt * s2;
      N = N + wt * st.n;
    }
  }

  // 7.
  if (!(W > 0.0f)) return out;
  DnPx cm;
  cm.r = Cr / W;
  cm.g = Cg / W;
  cm.b = Cb / W;
  cm.v = 0.0f;
  const float s2m = S / W;
  const float n = floorf(fminf(N / W, prm.max_history));
  if (!(n >= 1.0f)) return out;
  out.accum = RpRgb{cm.r * n, cm.g * n, cm.b * n};
  out.stats = RpStats{n, dn_lum(cm), s2m * (n - 1.0f), 0.0f};
  return out;
}

// Pixel (px, py) of the current frame: steps 1 and 2, then rp_history_px.
// guide_cur(x, y) returns the current frame's guide pixel (called once, for
// (px, py)).
template <class GuideCur, class GuidePrev, class AccumPrev, class StatsPrev>
PTMI_DN_HD RpOut rp_reproject_px(int32_t px, int32_t py, int32_t width, int32_t height, const RpCam& cur,
                                 const RpCam& prev, const RpParams& prm, GuideCur&& guide_cur, GuidePrev&& guide_prev,
                                 AccumPrev&& accum_prev, StatsPrev&& stats_prev) {
  // 1. the primary ray of ptmi_guide_trace
  const RpRay ray = rp_primary_ray(px, py, cur);

  // 2. the surface point seen from the previous camera, or the direction of a miss
  const DngG g = guide_cur(px, py);
  const bool hit_p = g.hit != 0.0f;
  RpV3 v = ray.d;
  if (hit_p) v = rp_sub(rp_surface_point(ray, g.z), rp_v3(prev.center));

  return rp_history_px(v, hit_p, g, width, height, prev, prm, guide_prev, accum_prev, stats_prev, RpEveryTap{});
}

}  // namespace ptmi
