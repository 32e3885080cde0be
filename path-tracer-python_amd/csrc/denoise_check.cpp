// denoise_check.cpp — the denoiser's per-pixel arithmetic (pt_denoise_math.hpp,
// the functions the kernels of pt_denoise.hip call) run on the CPU: a
// stand-alone host program, no HIP, no GPU. `make denoise_check` builds it;
// tests/test_denoise_abi.py compares its output with the numpy reference bit
// for bit.
//
//   denoise_check WIDTH HEIGHT ITERATIONS SIGMA accum.f32 stats.f32 rgb.f32 var.f32
//
// reads raw f32 accum (H x W x 3) and stats (H x W x 4), writes raw rgb
// (H x W x 3) and var (H x W). Exit 0 on success, 2 on bad arguments or I/O.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pt_denoise_math.hpp"

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
  if (argc != 9) {
    fprintf(stderr, "usage: %s WIDTH HEIGHT ITERATIONS SIGMA accum.f32 stats.f32 rgb.f32 var.f32\n", argv[0]);
    return 2;
  }
  const int32_t width = atoi(argv[1]), height = atoi(argv[2]), iterations = atoi(argv[3]);
  const float sigma = strtof(argv[4], nullptr);
  if (width < 1 || height < 1 || (int64_t)width * height > (1 << 26) || iterations < 0 ||
      iterations > kDnMaxIterations || !(sigma >= 0.0f)) {
    fprintf(stderr, "bad size, iterations or sigma\n");
    return 2;
  }
  const size_t npix = (size_t)width * (size_t)height;
  std::vector<float> accum(3 * npix), stats(4 * npix);
  if (!read_f32(argv[5], accum) || !read_f32(argv[6], stats)) {
    fprintf(stderr, "cannot read %zu pixels of accum and stats\n", npix);
    return 2;
  }
  std::vector<DnPx> a(npix), b(npix);
  for (size_t i = 0; i < npix; ++i)
    a[i] = dn_load_px(accum[3 * i], accum[3 * i + 1], accum[3 * i + 2], stats[4 * i], stats[4 * i + 2]);
  for (int32_t it = 0; it < iterations; ++it) {
    const DnPx* in = a.data();
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x)
        b[(size_t)y * width + x] = dn_pass_px(x, y, width, height, 1 << it, sigma, [&](int32_t qx, int32_t qy) {
          return in[(size_t)qy * width + qx];
        });
    a.swap(b);
  }
  std::vector<float> rgb(3 * npix), var(npix);
  for (size_t i = 0; i < npix; ++i) {
    rgb[3 * i] = a[i].r;
    rgb[3 * i + 1] = a[i].g;
    rgb[3 * i + 2] = a[i].b;
    var[i] = a[i].v;
  }
  if (!write_f32(argv[7], rgb) || !write_f32(argv[8], var)) {
    fprintf(stderr, "cannot write the outputs\n");
    return 2;
  }
  return 0;
}
