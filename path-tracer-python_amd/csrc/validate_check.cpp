// validate_check.cpp — the history validation's arithmetic
// (pt_validate_math.hpp, the functions the kernel of pt_validate.hip calls) run
// on the CPU: a stand-alone host program, no HIP, no GPU. `make validate_check`
// builds it; tests/test_validate_abi.py compares its output with the numpy
// reference bit for bit.
//
//   validate_check WIDTH HEIGHT in.f32 accum_out.f32 stats_out.f32 weight_out.f32
//
// in.f32 is raw little-endian f32: the parameters (radius, k_lo, k_hi: three
// values, the radius a whole number), then hist_accum (H x W x 3), hist_stats
// (H x W x 4), fresh_accum (H x W x 3) and fresh_stats (H x W x 4). Writes raw
// accum_out (H x W x 3), stats_out (H x W x 4) and weight_out (H x W). Step 1
// is computed once per pixel into an array, as the kernel stages it, and step 2
// reads it from there. Exit 0 on success, 2 on bad arguments or I/O.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/ptmi_validate.h"
#include "pt_check_io.hpp"
#include "pt_validate_math.hpp"

using namespace ptmi;

int main(int argc, char** argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: %s WIDTH HEIGHT in.f32 accum_out.f32 stats_out.f32 weight_out.f32\n", argv[0]);
    return 2;
  }
  const int32_t width = atoi(argv[1]), height = atoi(argv[2]);
  if (width < 1 || height < 1 || (int64_t)width * height > (1 << 26)) {
    fprintf(stderr, "bad size\n");
    return 2;
  }
  const size_t npix = (size_t)width * (size_t)height, head = 3;
  std::vector<float> in(head + (3 + 4 + 3 + 4) * npix);
  if (!read_f32(argv[3], in)) {
    fprintf(stderr, "cannot read the parameters and %zu pixels of four images\n", npix);
    return 2;
  }
  const float fr = in[0];
  if (!(fr >= 0.0f && fr <= (float)PTMI_VALIDATE_MAX_RADIUS) || fr != (float)(int32_t)fr || !dn_finite(in[1]) ||
      !dn_finite(in[2]) || !(in[1] >= 0.0f) || !(in[2] > in[1])) {
    fprintf(stderr, "bad parameters\n");
    return 2;
  }
  const VdParams prm = {(int32_t)fr, in[1], in[2]};
  const float* ha = in.data() + head;
  const float* hs = ha + 3 * npix;
  const float* fa = hs + 4 * npix;
  const float* fs = fa + 3 * npix;
  auto stats = [&](const float* s, size_t p) { return RpStats{s[4 * p], s[4 * p + 1], s[4 * p + 2], s[4 * p + 3]}; };
  auto rgb = [&](const float* a, size_t p) { return RpRgb{a[3 * p], a[3 * p + 1], a[3 * p + 2]}; };

  std::vector<VdEntry> entries(npix);
  for (size_t p = 0; p < npix; ++p) entries[p] = vd_entry(stats(hs, p), stats(fs, p));

  std::vector<float> accum(3 * npix), st(4 * npix), weight(npix);
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) {
      const VdSum sum = vd_window(x, y, width, height, prm.radius,
                                  [&](int32_t qx, int32_t qy) { return entries[(size_t)qy * width + qx]; });
      const float lam = vd_lambda(sum, prm.k_lo, prm.k_hi);
      const size_t p = (size_t)y * width + x;
      const VdOut o = vd_merge(rgb(ha, p), stats(hs, p), rgb(fa, p), stats(fs, p), lam);
      accum[3 * p] = o.accum.r;
      accum[3 * p + 1] = o.accum.g;
      accum[3 * p + 2] = o.accum.b;
      st[4 * p] = o.stats.n;
      st[4 * p + 1] = o.stats.mean;
      st[4 * p + 2] = o.stats.m2;
      st[4 * p + 3] = o.stats.pad;
      weight[p] = o.weight;
    }
  if (!write_f32(argv[4], accum) || !write_f32(argv[5], st) || !write_f32(argv[6], weight)) {
    fprintf(stderr, "cannot write the outputs\n");
    return 2;
  }
  return 0;
}
