// guide_check.cpp — the guided denoiser's per-pixel arithmetic
// (pt_guide_math.hpp, the functions the kernels of pt_guide.hip call) run on
// the CPU: a stand-alone host program, no HIP, no GPU. `make guide_check`
// builds it; tests/test_guide_abi.py compares its output with the numpy
// reference bit for bit.
//
//   guide_check WIDTH HEIGHT ITERATIONS SIGMA SIGMA_Z SIGMA_A NORMAL_POWER_LOG2 FLAGS
//               accum.f32 stats.f32 guides.f32 rgb.f32 var.f32
//
// reads raw f32 accum (H x W x 3), stats (H x W x 4) and guides (H x W x 8),
// writes raw rgb (H x W x 3) and var (H x W). Exit 0 on success, 2 on bad
// arguments or I/O.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pt_guide_math.hpp"

using namespace ptmi;

static bool read_f32(const char* path, std::vector<float>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), sizeof(float), v.size(), f);
  const bool at_end = fgetc(f) == EOF;
  fclose(f);
  return got == v.size() && at_end;
}

static bool write_f32(const char* path, const std::vector<float>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const size_t put = fwrite(v.data(), sizeof(float), v.size(), f);
  return fclose(f) == 0 && put == v.size();
}

int main(int argc, char** argv) {
  if (argc != 14) {
    fprintf(stderr,
            "usage: %s WIDTH HEIGHT ITERATIONS SIGMA SIGMA_Z SIGMA_A NORMAL_POWER_LOG2 FLAGS accum.f32 stats.f32 "
            "guides.f32 rgb.f32 var.f32\n",
            argv[0]);
    return 2;
  }
  const int32_t width = atoi(argv[1]), height = atoi(argv[2]), iterations = atoi(argv[3]);
  DngParams prm;
  prm.sigma = strtof(argv[4], nullptr);
  prm.sigma_z = strtof(argv[5], nullptr);
  prm.sigma_a = strtof(argv[6], nullptr);
  prm.normal_power_log2 = atoi(argv[7]);
  const int32_t flags = atoi(argv[8]);
  prm.demodulate = flags & 1;
  if (width < 1 || height < 1 || (int64_t)width * height > (1 << 26) || iterations < 0 ||
      iterations > kDnMaxIterations || !(prm.sigma >= 0.0f) || !(prm.sigma_z >= 0.0f) || !(prm.sigma_a >= 0.0f) ||
      prm.normal_power_log2 < 0 || prm.normal_power_log2 > kDngMaxNormalPower || (flags & ~1)) {
    fprintf(stderr, "bad size, iterations, sigmas, normal power or flags\n");
    return 2;
  }
  const size_t npix = (size_t)width * (size_t)height;
  std::vector<float> accum(3 * npix), stats(4 * npix), guides(8 * npix);
  if (!read_f32(argv[9], accum) || !read_f32(argv[10], stats) || !read_f32(argv[11], guides)) {
    fprintf(stderr, "cannot read %zu pixels of accum, stats and guides\n", npix);
    return 2;
  }
  std::vector<DngG> g(npix);
  for (size_t i = 0; i < npix; ++i) {
    const float* s = guides.data() + 8 * i;
    g[i] = DngG{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
  }
  std::vector<DnPx> a(npix), b(npix);
  for (size_t i = 0; i < npix; ++i)
    a[i] = dng_load_px(accum[3 * i], accum[3 * i + 1], accum[3 * i + 2], stats[4 * i], stats[4 * i + 2], g[i],
                       prm.demodulate);
  for (int32_t it = 0; it < iterations; ++it) {
    const DnPx* in = a.data();
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x)
        b[(size_t)y * width + x] = dng_pass_px(
            x, y, width, height, 1 << it, prm, [&](int32_t qx, int32_t qy) { return in[(size_t)qy * width + qx]; },
            [&](int32_t qx, int32_t qy) { return g[(size_t)qy * width + qx]; });
    a.swap(b);
  }
  std::vector<float> rgb(3 * npix), var(npix);
  for (size_t i = 0; i < npix; ++i) {
    const DnPx p = dng_store_px(a[i], g[i], prm.demodulate);
    rgb[3 * i] = p.r;
    rgb[3 * i + 1] = p.g;
    rgb[3 * i + 2] = p.b;
    var[i] = p.v;
  }
  if (!write_f32(argv[12], rgb) || !write_f32(argv[13], var)) {
    fprintf(stderr, "cannot write the outputs\n");
    return 2;
  }
  return 0;
}
