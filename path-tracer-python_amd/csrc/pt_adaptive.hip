// pt_adaptive.hip — per-pixel error estimates and the tile bookkeeping of
// adaptive sampling (DESIGN.md "Adaptive sampling").
//
//   * stats_resolve: stage_resolve (pt_megakernel.hip) plus a Welford update
//     of the sample luminance per pixel, {n, mean, M2, 0} in a second
//     per-pixel buffer, over all pixels of the frame or the pixels of a tile
//     list. Colours are added to accum in sample order exactly as
//     stage_resolve adds them, so accum stays bit-identical to a plain render.
//   * tile_error: one wave per 64-pixel megakernel tile reduces the pixels'
//     relative standard errors to a tile error and updates the tile's state.
//   * tile_compact: the active tiles' ids, ascending, and their count.
//
// All arithmetic is f32 with one rounding per operation (-ffp-contract=off,
// correctly rounded division and square root), so numpy f32 reproduces every
// value bit for bit.
#include "pt_launch.hpp"
#include "pt_prof.hpp"

namespace ptmi {

// accum[pixel] += staging[s][p] in sample order (stage_resolve) and the
// Welford update of the sample luminance in stats[pixel] = {n, mean, M2, 0}.
// LISTED: item i is lane i & 63 of tile tile_list[i >> 6]; pixels of unlisted
// tiles are neither read from staging nor written.
template <bool LISTED>
__global__ __launch_bounds__(kBlock) void stats_resolve(DevFrame fr, TileGrid g, const float* __restrict__ staging,
                                                        int32_t npix, int32_t batch, float* __restrict__ accum,
                                                        float* __restrict__ stats,
                                                        const int32_t* __restrict__ tile_list, int32_t nitems) {
  for (int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x); i < nitems; i += (int32_t)(gridDim.x * kBlock)) {
    int32_t p = i;  // unlisted: item i is flat pixel i of the frame
    size_t pix = LISTED ? 0 : frame_index(fr, i);
    if (LISTED) {
      const int32_t t = tile_list[i >> 6];
      int32_t lr, col;
      if ((uint32_t)t >= (uint32_t)g.ntiles) continue;  // ids outside the grid are ignored
      if (!tile_pixel(fr, g, t, i & 63, col, lr)) continue;
      p = lr * fr.w + col;
      pix = frame_index(fr, lr, col);
    }
    float* ap = accum + 3 * pix;
    float4* stp = reinterpret_cast<float4*>(stats) + pix;
    float a0 = ap[0], a1 = ap[1], a2 = ap[2];
    const float4 st = *stp;
    float n = st.x, mean = st.y, m2 = st.z;
    const float* sp = staging + 3 * (size_t)p;
    for (int32_t s = 0; s < batch; ++s) {
      const float* c = sp + 3 * (size_t)s * (size_t)npix;
      const float r = c[0], gr = c[1], b = c[2];
      a0 += r;
      a1 += gr;
      a2 += b;
      const float y = (0.2126f * r + 0.7152f * gr) + 0.0722f * b;
      const float n1 = n + 1.0f;
      const float d = y - mean;
      const float mean1 = mean + d / n1;
      m2 = m2 + d * (y - mean1);
      n = n1;
      mean = mean1;
    }
    ap[0] = a0;
    ap[1] = a1;
    ap[2] = a2;
    *stp = make_float4(n, mean, m2, st.w);  // [3] is reserved: kept as cleared
  }
}

hipError_t launch_stats_resolve(const DevFrame& fr, const float* staging, int32_t npix, int32_t batch, float* accum,
                                float* stats, const int32_t* tile_list, int32_t n_tiles, int prof_kind,
                                hipStream_t stream) {
  const TileGrid g = tile_grid(fr);
  const int64_t nitems = tile_list ? 64ll * n_tiles : (int64_t)npix;
  if (nitems <= 0) return hipSuccess;
  if (nitems > 0x7fffffff) return hipErrorInvalidValue;
  unsigned gr = (unsigned)((nitems + kBlock - 1) / kBlock);
  if (gr > 2048) gr = 2048;
  const int pslot = prof_begin(prof_kind, stream);
  if (tile_list)
    hipLaunchKernelGGL(stats_resolve<true>, dim3(gr), dim3(kBlock), 0, stream, fr, g, staging, npix, batch, accum,
                       stats, tile_list, (int32_t)nitems);
  else
    hipLaunchKernelGGL(stats_resolve<false>, dim3(gr), dim3(kBlock), 0, stream, fr, g, staging, npix, batch, accum,
                       stats, tile_list, (int32_t)nitems);
  prof_end(pslot, stream);
  return hipGetLastError();
}

// One wave per tile. Pixel error e = +inf for n < 2, else the relative
// standard error of the mean luminance, sqrt((M2 / (n - 1)) / n) / (|mean| +
// 0.01); lanes outside the frame contribute 0. The tile error E is the xor
// butterfly sum (offsets 32 .. 1) over (float)valid lanes. The cross-lane
// reads run with all 64 lanes active: every lane computes its value with
// selects and no lane leaves before the butterfly (DESIGN §4 "Cross-lane
// reads"); only whole waves past the last tile exit early.
// State (1 active, 0 done) is monotone: active' = active && n_tile < max_spp
// && (n_tile < min_spp || E > threshold), n_tile the n of lane 0's pixel.
// E > threshold is false for a NaN E, so a NaN sample ends its tile.
__global__ __launch_bounds__(kBlock) void tile_error(DevFrame fr, TileGrid g, const float* __restrict__ stats,
                                                     float threshold, float min_spp, float max_spp,
                                                     int32_t* __restrict__ tile_state, float* __restrict__ tile_err) {
  const int32_t lane = (int32_t)(threadIdx.x & 63u);
  const int32_t t = (int32_t)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));  // wave-uniform
  if (t >= g.ntiles) return;
  int32_t col, lr;
  const bool valid = tile_pixel(fr, g, t, lane, col, lr);
  float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (valid) st = reinterpret_cast<const float4*>(stats)[frame_index(fr, lr, col)];
  const float n = st.x;
  const float e = n < 2.0f ? __builtin_inff() : sqrtf((st.z / (n - 1.0f)) / n) / (fabsf(st.y) + 0.01f);
  float v = valid ? e : 0.0f;
  const unsigned long long mvalid = __ballot(valid);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  const float E = v / (float)__popcll(mvalid);
  const float n_tile = __shfl(n, 0, 64);  // lane 0 of a tile is always inside the frame
  if (lane == 0) {
    const bool more = n_tile < max_spp && (n_tile < min_spp || E > threshold);
    tile_err[t] = E;
    tile_state[t] = (tile_state[t] != 0 && more) ? 1 : 0;
  }
}

// Ordered compaction by one block: thread k owns a contiguous run of tiles,
// an exclusive scan of the runs' active counts gives each run's first output
// index, so the list is ascending (the megakernel's shards take list entries
// s, s + 8, ..: ascending ids keep that interleave spatial).
constexpr int kScanBlock = 1024;
__global__ __launch_bounds__(kScanBlock) void tile_compact(const int32_t* __restrict__ tile_state, int32_t ntiles,
                                                           int32_t* __restrict__ tile_list,
                                                           int32_t* __restrict__ n_active) {
  __shared__ int32_t part[kScanBlock];
  const int32_t k = (int32_t)threadIdx.x;
  const int32_t per = (ntiles + kScanBlock - 1) / kScanBlock;
  const int32_t lo = min(k * per, ntiles), hi = min(lo + per, ntiles);
  int32_t c = 0;
  for (int32_t t = lo; t < hi; ++t) c += tile_state[t] != 0 ? 1 : 0;
  part[k] = c;
  __syncthreads();
  for (int off = 1; off < kScanBlock; off <<= 1) {  // inclusive Hillis-Steele scan
    const int32_t add = k >= off ? part[k - off] : 0;
    __syncthreads();
    part[k] += add;
    __syncthreads();
  }
  int32_t o = part[k] - c;
  for (int32_t t = lo; t < hi; ++t)
    if (tile_state[t] != 0) tile_list[o++] = t;
  if (k == kScanBlock - 1) *n_active = part[k];
}

hipError_t launch_tile_update(const DevFrame& fr, const float* stats, float threshold, int32_t min_spp,
                              int32_t max_spp, int32_t* tile_state, float* tile_err, int32_t* tile_list,
                              int32_t* n_active, hipStream_t stream) {
  const TileGrid g = tile_grid(fr);
  if (g.ntiles <= 0) return hipMemsetAsync(n_active, 0, sizeof(int32_t), stream);
  const unsigned blocks = (unsigned)((g.ntiles + kBlock / 64 - 1) / (kBlock / 64));
  hipLaunchKernelGGL(tile_error, dim3(blocks), dim3(kBlock), 0, stream, fr, g, stats, threshold, (float)min_spp,
                     (float)max_spp, tile_state, tile_err);
  hipLaunchKernelGGL(tile_compact, dim3(1), dim3(kScanBlock), 0, stream, tile_state, g.ntiles, tile_list, n_active);
  return hipGetLastError();
}

}  // namespace ptmi
