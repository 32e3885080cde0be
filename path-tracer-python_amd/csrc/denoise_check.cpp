// denoise_check.cpp — the denoiser's per-pixel arithmetic (pt_denoise_math.hpp,
// the functions the kernels of pt_denoise.hip call) run on the CPU in both
// modes: a stand-alone host program, no HIP, no GPU. `make denoise_check` and
// `make guide_check` build it; tests/test_denoise_abi.py and
// tests/test_guide_abi.py compare its output with the numpy reference bit for
// bit.
//
//   denoise_check WIDTH HEIGHT ITERATIONS SIGMA accum.f32 stats.f32 rgb.f32 var.f32
//   denoise_check WIDTH HEIGHT ITERATIONS SIGMA SIGMA_Z SIGMA_A NORMAL_POWER_LOG2 FLAGS
//                 accum.f32 stats.f32 guides.f32 rgb.f32 var.f32
//
// reads raw f32 accum (H x W x 3) and stats (H x W x 4), in the second (guided)
// form guides (H x W x 8) as well, writes raw rgb (H x W x 3) and var (H x W).
// Exit 0 on success, 2 on bad arguments or I/O.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pt_check_io.hpp"
#include "pt_denoise_math.hpp"

using namespace ptmi;

template <bool GUIDED>
static void filter(int32_t width, int32_t height, int32_t iterations, const DngParams& prm, const float* accum,
                   const float* stats, const std::vector<DngG>& g, std::vector<float>& rgb, std::vector<float>& var) {
  const size_t npix = (size_t)width * (size_t)height;
  std::vector<DnPx> a(npix), b(npix);
  for (size_t i = 0; i < npix; ++i)
    a[i] = dng_load_px(accum[3 * i], accum[3 * i + 1], accum[3 * i + 2], stats[4 * i], stats[4 * i + 2],
                       GUIDED ? g[i] : DngG{}, GUIDED && prm.demodulate);
  for (int32_t it = 0; it < iterations; ++it) {
    const DnPx* in = a.data();
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x)
        b[(size_t)y * width + x] = dn_pass_px<GUIDED>(
            x, y, width, height, 1 << it, prm, [&](int32_t qx, int32_t qy) { return in[(size_t)qy * width + qx]; },
            [&](int32_t qx, int32_t qy) { return g[(size_t)qy * width + qx]; });
    a.swap(b);
  }
  for (size_t i = 0; i < npix; ++i) {
    const DnPx p = dng_store_px(a[i], GUIDED ? g[i] : DngG{}, GUIDED && prm.demodulate);
    rgb[3 * i] = p.r;
    rgb[3 * i + 1] = p.g;
    rgb[3 * i + 2] = p.b;
    var[i] = p.v;
  }
}

int main(int argc, char** argv) {
  if (argc != 9 && argc != 14) {
    fprintf(stderr,
            "usage: %s WIDTH HEIGHT ITERATIONS SIGMA [SIGMA_Z SIGMA_A NORMAL_POWER_LOG2 FLAGS] accum.f32 stats.f32 "
            "[guides.f32] rgb.f32 var.f32\n",
            argv[0]);
    return 2;
  }
  const bool guided = argc == 14;
  const int32_t width = atoi(argv[1]), height = atoi(argv[2]), iterations = atoi(argv[3]);
  DngParams prm = {};
  prm.sigma = strtof(argv[4], nullptr);
  int32_t flags = 0;
  if (guided) {
    prm.sigma_z = strtof(argv[5], nullptr);
    prm.sigma_a = strtof(argv[6], nullptr);
    prm.normal_power_log2 = atoi(argv[7]);
    flags = atoi(argv[8]);
    prm.demodulate = flags & 1;
  }
  if (width < 1 || height < 1 || (int64_t)width * height > (1 << 26) || iterations < 0 ||
      iterations > kDnMaxIterations || !(prm.sigma >= 0.0f) || !(prm.sigma_z >= 0.0f) || !(prm.sigma_a >= 0.0f) ||
      prm.normal_power_log2 < 0 || prm.normal_power_log2 > kDngMaxNormalPower || (flags & ~1)) {
    fprintf(stderr, "bad size, iterations, sigmas, normal power or flags\n");
    return 2;
  }
  char** files = argv + (guided ? 9 : 5);  // accum, stats, [guides,] rgb, var
  const size_t npix = (size_t)width * (size_t)height;
  std::vector<float> accum(3 * npix), stats(4 * npix), guides(guided ? 8 * npix : 0);
  if (!read_f32(files[0], accum) || !read_f32(files[1], stats) || (guided && !read_f32(files[2], guides))) {
    fprintf(stderr, "cannot read %zu pixels of accum, stats%s\n", npix, guided ? " and guides" : "");
    return 2;
  }
  std::vector<DngG> g(guided ? npix : 0);
  for (size_t i = 0; i < g.size(); ++i) {
    const float* s = guides.data() + 8 * i;
    g[i] = DngG{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
  }
  std::vector<float> rgb(3 * npix), var(npix);
  if (guided)
    filter<true>(width, height, iterations, prm, accum.data(), stats.data(), g, rgb, var);
  else
    filter<false>(width, height, iterations, prm, accum.data(), stats.data(), g, rgb, var);
  if (!write_f32(files[guided ? 3 : 2], rgb) || !write_f32(files[guided ? 4 : 3], var)) {
    fprintf(stderr, "cannot write the outputs\n");
    return 2;
  }
  return 0;
}
