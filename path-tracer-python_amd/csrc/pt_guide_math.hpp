// pt_guide_math.hpp — the per-pixel arithmetic of the guided a-trous denoiser
// (include/ptmi_guide.h states the contract), shared by the kernels of
// pt_guide.hip and the CPU check program guide_check.cpp. It is
// pt_denoise_math.hpp's filter (DnPx, dn_valid, dn_lum, dn_load_px) with the
// guide terms in the tap weight and the albedo demodulation around it.
//
// Host/device, no HIP type. A pixel's guides are DngG, the 32-byte guide pixel
// as two 16-byte halves: {nx, ny, nz, z} and {ar, ag, ab, hit}. Every operation
// is f32 with one rounding, in the order written here, so numpy f32 reproduces
// every value bit for bit (tests/guide_helpers.py).
#pragma once
#include "pt_denoise_math.hpp"

namespace ptmi {

struct alignas(16) DngG {
  float nx, ny, nz, z;
  float ar, ag, ab, hit;
};

struct DngParams {
  float sigma, sigma_z, sigma_a;
  int32_t normal_power_log2;
  int32_t demodulate;  // 0 or 1
};

constexpr float kDngAlbedoFloor = 1e-3f;
constexpr int kDngMaxNormalPower = 7;

// The demodulation divisor of a pixel: m per channel in r, g, b and lm * lm in v.
PTMI_DN_HD DnPx dng_modulation(const DngG& g) {
  DnPx m;
  m.r = fmaxf(g.ar, 0.0f) + kDngAlbedoFloor;
  m.g = fmaxf(g.ag, 0.0f) + kDngAlbedoFloor;
  m.b = fmaxf(g.ab, 0.0f) + kDngAlbedoFloor;
  m.v = 0.0f;
  const float lm = dn_lum(m);
  m.v = lm * lm;
  return m;
}

PTMI_DN_HD DnPx dng_load_px(float a0, float a1, float a2, float n, float m2, const DngG& g, int32_t demodulate) {
  DnPx p = dn_load_px(a0, a1, a2, n, m2);
  if (demodulate) {
    const DnPx m = dng_modulation(g);
    p.r = p.r / m.r;
    p.g = p.g / m.g;
    p.b = p.b / m.b;
    p.v = p.v / m.v;
  }
  return p;
}

PTMI_DN_HD DnPx dng_store_px(DnPx p, const DngG& g, int32_t demodulate) {
  if (demodulate) {
    const DnPx m = dng_modulation(g);
    p.r = p.r * m.r;
    p.g = p.g * m.g;
    p.b = p.b * m.b;
    p.v = p.v * m.v;
  }
  return p;
}

// The guide factors of a tap's weight: (tz * tz) * ((ta * ta) * wn) is formed by
// the caller in the contract's order; this returns them apart.
struct DngTerms {
  float tz, ta, wn;
};

PTMI_DN_HD DngTerms dng_terms(const DngG& p, const DngG& q, float den_z, float den_a, int32_t normal_power_log2) {
  DngTerms r;
  r.tz = fmaxf(0.0f, 1.0f - fabsf(p.z - q.z) / den_z);
  const float da = (fabsf(p.ar - q.ar) + fabsf(p.ag - q.ag)) + fabsf(p.ab - q.ab);
  r.ta = fmaxf(0.0f, 1.0f - da / den_a);
  float dn = fminf(1.0f, fmaxf(0.0f, (p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz));
  for (int32_t k = 0; k < normal_power_log2; ++k) dn = dn * dn;
  const bool hp = p.hit != 0.0f, hq = q.hit != 0.0f;
  r.wn = (hp && hq) ? dn : ((!hp && !hq) ? 1.0f : 0.0f);
  return r;
}

// One pass for pixel (x, y), as dn_pass_px: at(qx, qy) returns the pass's input
// pixel and guide(qx, qy) the guide pixel, for coordinates inside the image
// (neither is called for others; guide only for the centre and for valid taps).
template <class At, class Guide>
PTMI_DN_HD DnPx dng_pass_px(int32_t x, int32_t y, int32_t width, int32_t height, int32_t step, const DngParams& prm,
                            At&& at, Guide&& guide) {
  const DnPx p = at(x, y);
  if (!dn_valid(p)) return p;
  const float lp = dn_lum(p);
  const DngG gp = guide(x, y);

  // 3x3 prefiltered variance at unit spacing, for the luminance term only
  float vs = 0.0f, gs = 0.0f;
  for (int32_t dy = -1; dy <= 1; ++dy) {
    const int32_t qy = y + dy;
    if (qy < 0 || qy >= height) continue;
    const float gy = dy == 0 ? 0.5f : 0.25f;
    for (int32_t dx = -1; dx <= 1; ++dx) {
      const int32_t qx = x + dx;
      if (qx < 0 || qx >= width) continue;
      const DnPx q = at(qx, qy);
      if (!dn_valid(q)) continue;
      const float g = (dx == 0 ? 0.5f : 0.25f) * gy;
      vs = vs + g * q.v;
      gs = gs + g;
    }
  }
  const float vbar = vs / gs;
  const float den = prm.sigma * sqrtf(vbar) + kDnDenFloor;
  const float den_z = prm.sigma_z * gp.z + 1e-4f;
  const float den_a = prm.sigma_a + 1e-4f;

  float cr = 0.0f, cg = 0.0f, cb = 0.0f, vv = 0.0f, ws = 0.0f;
  for (int32_t dy = -2; dy <= 2; ++dy) {
    const int64_t qy = (int64_t)y + (int64_t)dy * step;
    if (qy < 0 || qy >= height) continue;
    const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
    for (int32_t dx = -2; dx <= 2; ++dx) {
      const int64_t qx = (int64_t)x + (int64_t)dx * step;
      if (qx < 0 || qx >= width) continue;
      const DnPx q = at((int32_t)qx, (int32_t)qy);
      if (!dn_valid(q)) continue;
      const DngG gq = guide((int32_t)qx, (int32_t)qy);
      const float h = (dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f)) * ky;
      const float xr = fabsf(lp - dn_lum(q)) / den;
      const float t = fmaxf(0.0f, 1.0f - xr);
      const DngTerms k = dng_terms(gp, gq, den_z, den_a, prm.normal_power_log2);
      const float w = ((h * (t * t)) * (k.tz * k.tz)) * ((k.ta * k.ta) * k.wn);
      cr = cr + w * q.r;
      cg = cg + w * q.g;
      cb = cb + w * q.b;
      vv = vv + (w * w) * q.v;
      ws = ws + w;
    }
  }
  DnPx o;
  o.r = cr / ws;
  o.g = cg / ws;
  o.b = cb / ws;
  o.v = vv / (ws * ws);
  return o;
}

}  // namespace ptmi
