// pt_mk_plan.hpp — the shape of a megakernel launch, decided on the host:
// the frame's 64-pixel tiles, the staged workspace, the 32-bit item-id limit
// and the work-unit plan of one staged batch; and the tile grid's inverse,
// the lane rule the kernels run (tile_col0, tile_row0, lane_col, lane_row,
// tile_pixel: host and device). Pure: no HIP runtime call and no kernel, so
// csrc/plan_check.cpp checks every plan, and the kernels' own lane rule, on
// the CPU. pt_megakernel.hip launches what mk_plan returns; pt_adaptive.hip
// and pt_abi.hip read the same tile grid.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_device.hpp"

namespace ptmi {

// Staged mode, persistent waves: the grid is one round of the chip's wave
// slots and every wave draws 64-item units (one 8x8 tile x one sample) from a
// device counter and refills its lanes across units — no wave ends while work
// is left, and there is no partly empty last round. Units are tile-major (all
// samples of a tile are consecutive), and a fetch takes up to
// PTMI_MK_CHUNK_SAMPLES units while plenty are left, fewer in the tail, so a
// wave changes tile rarely (lanes of two tiles in one wave fetch more distinct
// cache lines per load) and the last fetches are small.
#ifndef PTMI_MK_CHUNK_SAMPLES
#define PTMI_MK_CHUNK_SAMPLES 32  // A/B (C2, C4): 32/4 ~ 16/4 ~ 64/4 > 16/2, 16/8, 8/4 >> 64/2
#endif
#ifndef PTMI_MK_TAIL_DIV_SMALL
#define PTMI_MK_TAIL_DIV_SMALL 2  // ... for batches of fewer than PTMI_MK_SMALL_BATCH samples
#endif
#ifndef PTMI_MK_SMALL_BATCH
#define PTMI_MK_SMALL_BATCH 8000000
#endif
#ifndef PTMI_MK_SMALL_WPC
// Persistent waves per CU for a batch of fewer than PTMI_MK_SMALL_GRID_BATCH
// samples (the occupancy allows 20 for vol2): the next overlapped call's waves
// share the chip while this one drains. A/B on MI355X, an 8-rank tile shard's
// 64-spp calls against 20 waves per CU: 10 +1.1 %, 12 +0.6 %, 14 +0.5 %, 16
// -0.6 %, 8 -4 %, 6 -29 % (profiles/r06/ab/mk_small_grid.log; round 5:
// profiles/r05/ab/ab_mk_persist_wpc.log).
#define PTMI_MK_SMALL_WPC 10
#endif
#ifndef PTMI_MK_SMALL_GRID_BATCH
// Batches (samples) below which PTMI_MK_SMALL_WPC applies: 16 M covers the
// 4-rank tile shard (10.2 M samples per 64-spp call: +0.7 % over the full
// grid) and leaves 2-rank shards (20.5 M) and whole frames on the full grid
// (profiles/r06/ab/mk_small_grid.log).
#define PTMI_MK_SMALL_GRID_BATCH 16000000
#endif
#ifndef PTMI_MK_TAIL_DIV
#define PTMI_MK_TAIL_DIV 4  // a fetch takes at most (units left) / (TAIL_DIV * waves) units
                            // (re-tuned: 2 is +3 % on C2 but -8 % on C4's long fog paths;
                            // profiles/r01/ab_fetch_sizing.log)
#endif

// Unit counters: the units are split into PTMI_MK_SHARDS contiguous shards,
// each with its own counter on its own 256-B line, and wave w pulls from shard
// w % PTMI_MK_SHARDS first (one shard per XCD under round-robin placement),
// then steals from the others. One device-scope counter saturates near 88
// returning atomics per us (MI355X_MICROARCH.md, "dequeue"), and a launch
// makes ~10^5 fetches, most of them small ones in its tail, where every wave
// is waiting for its next unit.
#ifndef PTMI_MK_SHARDS
#define PTMI_MK_SHARDS 8
#endif
// Shard s holds tiles s, s + S, s + 2S, ... (interleaved across the image, so
// every shard costs about the same; 0: contiguous unit ranges, whose shards
// drain at different times). A/B on MI355X, C2, 64-spp calls (overlapped):
// one counter 2448 (2479), 8 contiguous shards 2320 (2546), 8 interleaved
// 2560 (2597), 4 interleaved 2552 (2590) Msamples/s; 16-spp calls 1954 ->
// 2324 (profiles/r02/ab/ab_mk_shards.log).
constexpr int kMkShards = PTMI_MK_SHARDS;
constexpr int kMkCtlLine = 64;  // int32 words per 256-B counter line

struct MkWork {
  int32_t* ctl;      // kMkShards counters, one per 256-B line: units taken from each shard (zeroed before the launch)
  int32_t shard_len; // units per shard (the last one may be short)
  int32_t csamp;     // most units per fetch
  int32_t tiles_x;   // 64-pixel tiles per row
  int32_t tw_log2;   // tile width log2: 3 for 8x8 tiles, 4 for 16x4, 5 for 32x2, 6 for 64x1
  int32_t nb;        // samples of the batch (units per tile)
  FastDiv by_nb, by_tiles_x, by_len;
  int32_t nunits;    // units of the batch (multiple of csamp)
  int32_t tail_div;  // TAIL_DIV * waves of the grid
  // tile-listed launches (mk_render_kernel's LISTED): the batch's virtual tile
  // v is tile tile_list[v]; v >= n_list or an id outside [0, ntiles) decodes
  // outside the frame, as the shards' padded units do
  const int32_t* tile_list;
  int32_t n_list, ntiles;
};

// The frame's 64-pixel tiles, as the staged megakernel and the adaptive
// kernels (pt_adaptive.hip) number them.
struct TileGrid {
  int32_t tw_log2;  // tile width log2 (3: 8x8, 4: 16x4, 5: 32x2, 6: 64x1)
  int32_t tiles_x, ntiles;
};

// A frame's local rows are its row bands packed together, so an 8x8 tile over
// 4-row bands (bench.py --gpus 8 at 800 rows) would cover two runs of 4 image
// rows 32 rows apart; a tile as tall as the band's largest power-of-two
// divisor (16x4, 32x2, 64x1) stays inside one band. Which lane renders which
// pixel changes nothing in the image (staging[sample][pixel], ordered resolve).
inline TileGrid tile_grid(const DevFrame& fr) {
  int th_log2 = 3;
  if (fr.band_stride > 1) {
    const int32_t th = fr.band_rows & -fr.band_rows;
    th_log2 = th >= 8 ? 3 : th >= 4 ? 2 : th >= 2 ? 1 : 0;
  }
  const int32_t tw = 64 >> th_log2, th = 1 << th_log2;
  TileGrid g;
  g.tw_log2 = 6 - th_log2;
  g.tiles_x = (fr.w + tw - 1) / tw;
  g.ntiles = g.tiles_x * ((fr.n_rows + th - 1) / th);  // <= pixels of the image: fits
  return g;
}

// The lane rule, stated here only: tile (tx, ty) of a grid of 1 << tw_log2
// wide tiles starts at window column tx << tw_log2 and local row
// ty << (6 - tw_log2), and lane p of a tile lies p & (tw - 1) columns and
// p >> tw_log2 rows from there. Splitting a tile id into (tx, ty) is the
// caller's (plain division in tile_pixel, FastDiv in the render kernels).
// (One value per function: a caller keeps its own order of evaluation, and
// with it the device code it had.)
__host__ __device__ __forceinline__ int32_t tile_col0(int32_t tw_log2, int32_t tx) { return tx << tw_log2; }
__host__ __device__ __forceinline__ int32_t tile_row0(int32_t tw_log2, int32_t ty) { return ty << (6 - tw_log2); }
__host__ __device__ __forceinline__ int32_t lane_col(int32_t tw_log2, int32_t p) { return p & ((1 << tw_log2) - 1); }
__host__ __device__ __forceinline__ int32_t lane_row(int32_t tw_log2, int32_t p) { return p >> tw_log2; }

// Lane p of tile t -> the pixel's column in the window and its local row;
// false outside the frame.
__host__ __device__ __forceinline__ bool tile_pixel(const DevFrame& fr, const TileGrid& g, int32_t t, int32_t p,
                                                    int32_t& col, int32_t& lr) {
  const int32_t ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
  col = tile_col0(g.tw_log2, tx) + lane_col(g.tw_log2, p);
  lr = tile_row0(g.tw_log2, ty) + lane_row(g.tw_log2, p);
  return col < fr.w && lr < fr.n_rows;
}

// The staged workspace: staging[sample][pixel][3], then the shards' counter lines.
struct MkWorkspace {
  size_t staging;    // bytes of staging, a multiple of 256: the counter lines' offset
  size_t ctl_bytes;  // kMkShards 256-B lines
  size_t total;
};
inline MkWorkspace mk_workspace(int32_t npix, int32_t batch) {
  MkWorkspace w;
  w.staging = (3 * sizeof(float) * (size_t)npix * (size_t)batch + 255) & ~(size_t)255;
  w.ctl_bytes = sizeof(int32_t) * kMkCtlLine * kMkShards;
  w.total = w.staging + w.ctl_bytes;
  return w;
}
inline size_t mk_workspace_bytes(int32_t npix, int32_t batch) {
  return npix > 0 && batch > 0 ? mk_workspace(npix, batch).total : 0;
}

// Item ids (unit, lane of the 64-pixel tile) are 32-bit, and the interleaved
// shards number virtual units up to a whole tile per shard past the last one:
// the most samples nb with padded tiles * nb * 64 < 2^32 (0: no tile).
inline int64_t mk_padded_tiles(int64_t tiles) { return (tiles + kMkShards - 1) / kMkShards * kMkShards; }
inline int64_t mk_max_batch_of(int64_t tiles) {
  return tiles > 0 ? ((1ll << 32) - 1) / (mk_padded_tiles(tiles) * 64) : 0;
}
inline int64_t mk_max_batch(const DevFrame& fr) { return mk_max_batch_of(tile_grid(fr).ntiles); }

// One staged batch of nb samples into the workspace at ws: the kernel's work
// description, its grid (persistent one-wave blocks) and the bytes to zero at
// wk.ctl before the launch. tile_list != nullptr: the units cover the n_list
// listed tiles only. per_cu: the kernel's occupancy in blocks per CU; ncu: CUs.
struct MkPlan {
  MkWork wk;
  unsigned waves;
  size_t ctl_bytes;
  hipError_t err;  // hipErrorInvalidValue: the batch's item ids do not fit 32 bits
};
inline MkPlan mk_plan(const DevFrame& fr, void* ws, int32_t nb, const int32_t* tile_list, int32_t n_list,
                      int per_cu, int ncu) {
  MkPlan P{};
  const TileGrid g = tile_grid(fr);
  const int64_t tiles = tile_list ? (int64_t)n_list : (int64_t)g.ntiles;  // tiles the units cover
  if (nb < 1 || nb > mk_max_batch_of(tiles)) {
    P.err = hipErrorInvalidValue;
    return P;
  }
  const int64_t batch_samples = (tile_list ? 64 * tiles : (int64_t)fr.w * fr.n_rows) * nb;
  const MkWorkspace w = mk_workspace(fr.w * fr.n_rows, nb);
  MkWork& wk = P.wk;
  wk.ctl = (int32_t*)((char*)ws + w.staging);
  wk.csamp = PTMI_MK_CHUNK_SAMPLES;
  wk.tiles_x = g.tiles_x;
  wk.tw_log2 = g.tw_log2;
  wk.nb = nb;
  wk.tile_list = tile_list;
  wk.n_list = n_list;
  wk.ntiles = g.ntiles;
  // shard s: tiles s, s + S, ... (interleaved across the image, so every shard
  // costs about the same); virtual units past the last tile decode to rows
  // outside the frame and are skipped
  wk.shard_len = (int32_t)(mk_padded_tiles(tiles) / kMkShards) * nb;
  wk.nunits = wk.shard_len * kMkShards;
  wk.by_len = fast_div((uint32_t)wk.shard_len);
  wk.by_nb = fast_div((uint32_t)nb);
  wk.by_tiles_x = fast_div((uint32_t)wk.tiles_x);
  // Small batches (an 8-rank tile shard) run on a smaller persistent grid, so
  // the next overlapped call's waves share the chip while this one drains.
  if (batch_samples < PTMI_MK_SMALL_GRID_BATCH && per_cu > PTMI_MK_SMALL_WPC) per_cu = PTMI_MK_SMALL_WPC;
  int64_t waves = (int64_t)(per_cu > 0 ? per_cu : 1) * (ncu > 0 ? ncu : 1);
  if (waves > wk.nunits) waves = wk.nunits;
  // per shard: the waves pulling from it. Small batches (a multi-GPU tile
  // shard: 5 M samples per call for vol2 at 8 GPUs) are all tail: halving the
  // divisor there takes larger fetches, so a wave changes tile less often
  // (A/B, 8-rank rehearsal: +2 % per GPU; profiles/r03/ab/ab_mk_small_calls.log).
  const int64_t tail = batch_samples < PTMI_MK_SMALL_BATCH ? PTMI_MK_TAIL_DIV_SMALL : PTMI_MK_TAIL_DIV;
  const int64_t tdiv = tail * waves / kMkShards;
  wk.tail_div = (int32_t)(tdiv > 1 ? tdiv : 1);
  P.waves = (unsigned)waves;
  P.ctl_bytes = w.ctl_bytes;
  P.err = hipSuccess;
  return P;
}

}  // namespace ptmi
