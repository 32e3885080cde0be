// pt_validate_math.hpp — the arithmetic of the history validation
// (include/ptmi_validate.h states the contract), one function per step, shared
// by the kernel of pt_validate.hip and the CPU check program
// validate_check.cpp.
//
// Host/device, no HIP type. A stats pixel and an accum pixel are
// pt_reproject_math.hpp's RpStats and RpRgb; the caller decides where they are
// read from (the kernel stages step 1 in LDS and reads step 2's window from
// there). Every operation is f32 with one rounding, in the order written here,
// so numpy f32 reproduces every value bit for bit (tests/validate_helpers.py).
#pragma once
#include "pt_reproject_math.hpp"

namespace ptmi {

struct VdParams {
  int32_t radius;
  float k_lo, k_hi;
};

constexpr int32_t kVdMaxRadius = 7;  // PTMI_VALIDATE_MAX_RADIUS

struct VdEntry {  // step 1 of one pixel
  float d, v;
  uint32_t usable;
};

struct VdSum {  // step 2 of one window
  float D, V;
  uint32_t m;
};

struct VdOut {
  RpRgb accum;
  RpStats stats;
  float weight;
};

// Step 1: the difference of the two means of a pixel and its variance.
PTMI_DN_HD VdEntry vd_entry(const RpStats& h, const RpStats& f) {
  VdEntry e = {0.0f, 0.0f, 0u};
  if (!(h.n >= 2.0f && f.n >= 2.0f)) return e;
  if (!(dn_finite(h.n) && dn_finite(h.mean) && dn_finite(h.m2) && dn_finite(f.n) && dn_finite(f.mean) &&
        dn_finite(f.m2)))
    return e;
  e.d = f.mean - h.mean;
  e.v = (h.m2 / (h.n - 1.0f)) / h.n + (f.m2 / (f.n - 1.0f)) / f.n;
  e.usable = 1u;
  return e;
}

// Step 2: the sums over the window of (x, y), clipped to the image, j outer
// and i inner. entry(qx, qy) returns step 1 of a pixel inside the image.
template <class Entry>
PTMI_DN_HD VdSum vd_window(int32_t x, int32_t y, int32_t width, int32_t height, int32_t radius, Entry&& entry) {
  VdSum s = {0.0f, 0.0f, 0u};
  for (int32_t j = -radius; j <= radius; ++j) {
    const int32_t qy = y + j;
    if (qy < 0 || qy >= height) continue;
    for (int32_t i = -radius; i <= radius; ++i) {
      const int32_t qx = x + i;
      if (qx < 0 || qx >= width) continue;
      const VdEntry e = entry(qx, qy);
      s.D = s.D + e.d;
      s.V = s.V + e.v;
      s.m += e.usable;
    }
  }
  return s;
}

// Step 3: the stale fraction of a window.
PTMI_DN_HD float vd_lambda(const VdSum& s, float k_lo, float k_hi) {
  if (s.m == 0u) return 0.0f;
  if (s.D != s.D || s.V != s.V) return 1.0f;
  if (s.V > 0.0f) {
    const float z = fabsf(s.D) / sqrtf(s.V);
    if (z != z) return 1.0f;
    return fminf(fmaxf((z - k_lo) / (k_hi - k_lo), 0.0f), 1.0f);
  }
  if (s.V == 0.0f) return s.D == 0.0f ? 0.0f : 1.0f;
  return 1.0f;
}

// Steps 4 - 6 of a pixel whose window's stale fraction is lam.
PTMI_DN_HD VdOut vd_merge(RpRgb ha, RpStats hs, const RpRgb& fa, const RpStats& fs, float lam) {
  // 4.
  if (!(dn_finite(ha.r) && dn_finite(ha.g) && dn_finite(ha.b) && dn_finite(hs.n) && dn_finite(hs.mean) &&
        dn_finite(hs.m2))) {
    ha = RpRgb{0.0f, 0.0f, 0.0f};
    hs = RpStats{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const float n_h = hs.n;
  const float n_v = floorf(n_h * (1.0f - lam));

  VdOut o;
  o.weight = n_h >= 1.0f ? n_v / n_h : 0.0f;  // 6.

  // 5.
  if (!(n_v >= 1.0f)) {
    o.accum = fa;
    o.stats = fs;
    return o;
  }
  RpRgb av = ha;
  float m2_v = hs.m2;
  if (n_v != n_h) {
    const float scale = (float)(1.0 / (double)fmaxf(n_h, 1.0f));
    av = RpRgb{(ha.r * scale) * n_v, (ha.g * scale) * n_v, (ha.b * scale) * n_v};
    m2_v = n_h >= 2.0f ? (hs.m2 / (n_h - 1.0f)) * (n_v - 1.0f) : 0.0f;
  }
  if (fs.n == 0.0f) {
    o.accum = av;
    o.stats = RpStats{n_v, hs.mean, m2_v, 0.0f};
    return o;
  }
  const float delta = fs.mean - hs.mean;
  const float n = n_v + fs.n;
  o.accum = RpRgb{av.r + fa.r, av.g + fa.g, av.b + fa.b};
  o.stats = RpStats{n, hs.mean + delta * (fs.n / n), (m2_v + fs.m2) + (delta * delta) * ((n_v * fs.n) / n), 0.0f};
  return o;
}

}  // namespace ptmi
