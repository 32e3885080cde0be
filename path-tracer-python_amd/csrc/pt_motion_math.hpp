// pt_motion_math.hpp — step 2' of the motion-aware reprojection
// (include/ptmi_motion.h states the contract): the id decode and, per primitive
// type, the place a surface point had on its primitive before a scene update.
// Shared by the kernel of pt_motion.hip and the CPU check program
// motion_check.cpp; steps 3 - 7 are pt_reproject_math.hpp's rp_history_px.
//
// Host/device, no HIP type. A row is the primitive's f32 row of include/ptmi.h
// (4, 16 or 12 values); the caller decides where it is read from, after
// mv_decode has checked the id against the counts. Every operation is f32 with
// one rounding, in the order written here, so numpy f32 reproduces every value
// bit for bit (tests/motion_helpers.py).
#pragma once
#include "pt_reproject_math.hpp"

namespace ptmi {

enum : int32_t { kMvSphere = 0, kMvTriangle = 1, kMvQuad = 2 };  // the leaf type codes of include/ptmi.h
constexpr int32_t kMvSphereFloats = 4, kMvQuadFloats = 16, kMvTriFloats = 12;
constexpr int32_t kMvMaxPrims = 1 << 25;  // prim index < 2^25 per type (include/ptmi.h)

struct MvCounts {
  int32_t spheres, quads, tris;
};

struct MvId {
  int32_t type, prim;
};

// The id of a pixel that has a row to read: false for -1 (any negative id), an
// unknown type, and a prim at or past the count of its type. Nothing may be
// addressed through an id this rejects.
PTMI_DN_HD bool mv_decode(int32_t id, const MvCounts& n, MvId& out) {
  if (id < 0) return false;
  out.type = id >> 28;  // 0 .. 7
  out.prim = id & 0x0fffffff;
  const int32_t count = out.type == kMvSphere ? n.spheres : out.type == kMvQuad ? n.quads
                        : out.type == kMvTriangle ? n.tris : 0;
  return out.prim < count;
}

PTMI_DN_HD uint32_t mv_bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, sizeof u);
  return u;
}

template <int N>
PTMI_DN_HD bool mv_same_row(const float (&a)[N], const float (&b)[N]) {
  bool same = true;
  for (int k = 0; k < N; ++k) same = same && mv_bits(a[k]) == mv_bits(b[k]);
  return same;
}

PTMI_DN_HD RpV3 mv_add(RpV3 a, RpV3 b) { return RpV3{a.x + b.x, a.y + b.y, a.z + b.z}; }
PTMI_DN_HD RpV3 mv_scale(RpV3 a, float s) { return RpV3{a.x * s, a.y * s, a.z * s}; }

// Sphere, row {c, r}: the same direction from the centre, at the same fraction of the radius.
PTMI_DN_HD RpV3 mv_sphere_prev(RpV3 P, const float (&cur)[kMvSphereFloats], const float (&old)[kMvSphereFloats]) {
  if (mv_same_row(cur, old)) return P;
  const float k = old[3] / cur[3];
  return mv_add(rp_v3(old), mv_scale(rp_sub(P, rp_v3(cur)), k));
}

// Quad, row {n, D, Q, u, v, w}: the same (alpha, beta), as hit_quad forms them.
PTMI_DN_HD RpV3 mv_quad_prev(RpV3 P, const float (&cur)[kMvQuadFloats], const float (&old)[kMvQuadFloats]) {
  if (mv_same_row(cur, old)) return P;
  const RpV3 h = rp_sub(P, rp_v3(cur + 4));
  const RpV3 w = rp_v3(cur + 13);
  const float alpha = rp_dot(w, rp_cross(h, rp_v3(cur + 10)));
  const float beta = rp_dot(w, rp_cross(rp_v3(cur + 7), h));
  return mv_add(mv_add(rp_v3(old + 4), mv_scale(rp_v3(old + 7), alpha)), mv_scale(rp_v3(old + 10), beta));
}

// Triangle, row {v0, e1, e2, n}: the same barycentric coordinates.
PTMI_DN_HD RpV3 mv_tri_prev(RpV3 P, const float (&cur)[kMvTriFloats], const float (&old)[kMvTriFloats]) {
  if (mv_same_row(cur, old)) return P;
  const RpV3 e1 = rp_v3(cur + 3), e2 = rp_v3(cur + 6);
  const RpV3 h = rp_sub(P, rp_v3(cur));
  const RpV3 m = rp_cross(e1, e2);
  const float mm = rp_dot(m, m);
  const float alpha = rp_dot(rp_cross(h, e2), m) / mm;
  const float beta = rp_dot(rp_cross(e1, h), m) / mm;
  return mv_add(mv_add(rp_v3(old), mv_scale(rp_v3(old + 3), alpha)), mv_scale(rp_v3(old + 6), beta));
}

// Pixel (px, py) of the current frame: steps 1 and 2', then rp_history_px with
// step 5's tap condition. guide_cur and id_cur are called once, for (px, py);
// id_prev(x, y) for taps inside the image, with match_ids only.
// prev_point(P, id) returns P_prev for an id mv_decode accepted (it reads the
// primitive's two rows and calls mv_sphere_prev, mv_quad_prev or mv_tri_prev)
// and is called for no other id.
template <class GuideCur, class IdCur, class PrevPoint, class GuidePrev, class AccumPrev, class StatsPrev,
          class IdPrev>
PTMI_DN_HD RpOut mv_reproject_px(int32_t px, int32_t py, int32_t width, int32_t height, const RpCam& cur,
                                 const RpCam& prev, const RpParams& prm, bool match_ids, const MvCounts& counts,
                                 GuideCur&& guide_cur, IdCur&& id_cur, PrevPoint&& prev_point,
                                 GuidePrev&& guide_prev, AccumPrev&& accum_prev, StatsPrev&& stats_prev,
                                 IdPrev&& id_prev) {
  const RpRay ray = rp_primary_ray(px, py, cur);
  const DngG g = guide_cur(px, py);
  const bool hit_p = g.hit != 0.0f;
  RpV3 v = ray.d;
  int32_t id = -1;
  if (hit_p) {
    const RpV3 P = rp_surface_point(ray, g.z);
    id = id_cur(px, py);
    MvId m;
    if (!mv_decode(id, counts, m)) return RpOut{};  // no history, and no row read
    v = rp_sub(prev_point(P, m), rp_v3(prev.center));
  }
  return rp_history_px(v, hit_p, g, width, height, prev, prm, guide_prev, accum_prev, stats_prev,
                       [&](int32_t qx, int32_t qy) { return !match_ids || id_prev(qx, qy) == id; });
}

}  // namespace ptmi
