// pt_denoise_math.hpp — the per-pixel arithmetic of the a-trous denoiser in
// both of its modes: variance-guided (include/ptmi_post.h states the contract)
// and guided by the first-hit guide buffers as well (include/ptmi_guide.h).
// Shared by the kernels of pt_denoise.hip and the CPU check program
// denoise_check.cpp.
//
// Host/device, no HIP type: a pixel of the working image is DnPx {r, g, b, v}
// (the kernels move it as one float4), a pixel's guides are DngG, the 32-byte
// guide pixel as two 16-byte halves: {nx, ny, nz, z} and {ar, ag, ab, hit}.
// Every operation is f32 with one rounding (-ffp-contract=off, correctly
// rounded / and sqrtf), in the order written here, so numpy f32 reproduces
// every value bit for bit (tests/denoise_helpers.py).
//
// Validity is a property of a working pixel as a pass reads it: its luminance
// and its variance are finite. Invalid pixels are copied through and are
// skipped as taps, so they stay as they are from dn_load_px to the output.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PTMI_DN_HD __host__ __device__ __forceinline__
#else
#define PTMI_DN_HD inline
#endif

namespace ptmi {

struct alignas(16) DnPx {
  float r, g, b, v;
};

struct alignas(16) DngG {
  float nx, ny, nz, z;
  float ar, ag, ab, hit;
};

// The unguided filter reads sigma only.
struct DngParams {
  float sigma, sigma_z, sigma_a;
  int32_t normal_power_log2;
  int32_t demodulate;  // 0 or 1
};

constexpr float kDnUnknownVar = 1e10f;  // n < 2: "unknown, trust the neighbours"
constexpr float kDnDenFloor = 1e-4f;
constexpr int kDnMaxIterations = 8;
constexpr float kDngAlbedoFloor = 1e-3f;
constexpr int kDngMaxNormalPower = 7;

PTMI_DN_HD bool dn_finite(float x) { return fabsf(x) <= FLT_MAX; }

PTMI_DN_HD float dn_lum(const DnPx& p) { return (0.2126f * p.r + 0.7152f * p.g) + 0.0722f * p.b; }

PTMI_DN_HD bool dn_valid(const DnPx& p) { return dn_finite(dn_lum(p)) && dn_finite(p.v); }

// accum[p] and stats[p] = {n, mean, M2, .} to the working pixel: the colour
// scaled as ptmi_tonemap_stats scales it, and the variance of the mean
// luminance.
PTMI_DN_HD DnPx dn_load_px(float a0, float a1, float a2, float n, float m2) {
  const float scale = (float)(1.0 / (double)(n > 1.0f ? n : 1.0f));
  DnPx p;
  p.r = a0 * scale;
  p.g = a1 * scale;
  p.b = a2 * scale;
  p.v = n >= 2.0f ? (m2 / (n - 1.0f)) / n : kDnUnknownVar;
  return p;
}

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

// One pass for pixel (x, y) of a width x height image with tap spacing `step`:
// at(qx, qy) returns the pass's input pixel for coordinates inside the image
// (it is never called for others). GUIDED: guide(qx, qy) returns the guide
// pixel, called for the centre and for valid taps only; unguided it is never
// called and the tap weight is h * (t * t) alone.
template <bool GUIDED, class At, class Guide>
PTMI_DN_HD DnPx dn_pass_px(int32_t x, int32_t y, int32_t width, int32_t height, int32_t step, const DngParams& prm,
                           At&& at, Guide&& guide) {
  const DnPx p = at(x, y);
  if (!dn_valid(p)) return p;
  const float lp = dn_lum(p);
  DngG gp = {};
  if constexpr (GUIDED) gp = guide(x, y);

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
  float den_z = 0.0f, den_a = 0.0f;
  if constexpr (GUIDED) {
    den_z = prm.sigma_z * gp.z + 1e-4f;
    den_a = prm.sigma_a + 1e-4f;
  }

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
      DngG gq = {};
      if constexpr (GUIDED) gq = guide((int32_t)qx, (int32_t)qy);
      const float h = (dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f)) * ky;
      const float xr = fabsf(lp - dn_lum(q)) / den;
      const float t = fmaxf(0.0f, 1.0f - xr);
      float w;
      if constexpr (GUIDED) {
        const DngTerms k = dng_terms(gp, gq, den_z, den_a, prm.normal_power_log2);
        w = ((h * (t * t)) * (k.tz * k.tz)) * ((k.ta * k.ta) * k.wn);
      } else {
        w = h * (t * t);
      }
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

// 2 working images of 16 B per pixel, rounded up to 256 B.
inline size_t dn_workspace_bytes(int64_t npix) { return (size_t)((2 * 16 * npix + 255) / 256 * 256); }

}  // namespace ptmi
