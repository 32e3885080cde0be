// pt_wf_plan.hpp — the shape of a wavefront batch, decided on the host: the
// workspace carved into every pipe's buffers, the batch's work items, the
// grids and the id limit; and the plan's inverse, the work-item decode the
// kernels run (decode_item: host and device). Pure: no HIP runtime call and no
// kernel, so csrc/plan_check.cpp checks every plan, and the kernels' own
// decode of it, on the CPU. pt_wavefront.hip launches what wf_plan returns.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_device.hpp"
#include "pt_mk_plan.hpp"

namespace ptmi {

constexpr int kShards = 8;
#ifndef PTMI_WF_CHUNK_SAMPLES
#define PTMI_WF_CHUNK_SAMPLES 4  // samples per work chunk (one 8x8 pixel square each)
#endif
#ifndef PTMI_WF_BLOCK
#define PTMI_WF_BLOCK 128  // threads per block of the queue kernels (A/B on MI355X, parity-identical: 128 vs 256
                           // C3 +1.2 %, mesh fog +1.7 %; 64: C3 -6 %, mesh fog +2.3 %; profiles/r02/ab/ab_wf_block.log)
#endif
constexpr int kWfBlock = PTMI_WF_BLOCK;
#ifndef PTMI_WF_ISECT_LDS
// Stack slots wf_intersect keeps in LDS when its stack is deeper than 16
// slots; the deeper slots spill to global memory (Stack, pt_device.hpp). Its
// LDS stacks set its occupancy: the 20-slot kernel (leaf depth 16-19, e.g.
// the mesh-fog torus) fits 4 waves/SIMD with all slots in LDS, 7 with 11
// (67 VGPRs). A/B on MI355X, parity-identical (also with 3 LDS slots, where
// most pushes spill): mesh fog +2.2 %; for the 16-slot kernel (vol2, C3) 7
// waves measured -1.5 % on round 3's in-place slots (profiles/r03/ab/ab_wf_spill.log)
// and +0.8 % on round 5's compacted buffers (PTMI_WF_SPILL_MIN_STACK,
// pt_wavefront.hip). A 16-slot wf_intersect padded down to 4 waves/SIMD loses
// 8 % (3 waves: 18 %).
#define PTMI_WF_ISECT_LDS 10
#endif
#ifndef PTMI_WF_SPILL_MAX_STACK
#define PTMI_WF_SPILL_MAX_STACK 20  // kernels of 17 to this many stack slots spill; deeper ones keep them all in LDS
#endif
constexpr int kSpillSlots = PTMI_WF_SPILL_MAX_STACK > PTMI_WF_ISECT_LDS ? PTMI_WF_SPILL_MAX_STACK - PTMI_WF_ISECT_LDS : 0;
#ifndef PTMI_WF_MAX_BLOCKS
#define PTMI_WF_MAX_BLOCKS (2048 * 256 / PTMI_WF_BLOCK)  // all pipes together; A/B: 4096 -1.5 %, 8192 -3.5 % (C3)
#endif

// Continuing-ray segments: kBins direction bins x kShards producer shards,
// one counter each (kSegs <= 64: one wave holds them all, one per lane).
// Sorting by octant, A/B on MI355X (round 5, parity-identical;
// profiles/r05/ab/ab_wf_sort.log): against the round-4 in-place slots
// (1685-1694 Msamples/s on C3, 705-708 on mesh fog) the compacted buffers
// alone (one bin) give 1889-1900 / 847-849, sorted by octant 1914-1923 /
// 850-854; wf_intersect's lane efficiency 0.43 unsorted, 0.45 sorted.
constexpr int kBins = 8;
constexpr int kSegs = kBins * kShards;
#ifndef PTMI_WF_SEG_DIV
#define PTMI_WF_SEG_DIV 16  // a segment's region holds capacity / this rays (4x an even share of 64 segments)
#endif

// Ray buffer of one iteration parity: positions [0, npos) of six streams.
// Segment s holds positions [s * seg_cap, (s + 1) * seg_cap), the overflow
// region the next `capacity`, the fresh camera rays the last `capacity`.
struct RayBuf {
  float4* a;       // o.xyz, d.x
  float4* c;       // thr.xyz, meta (bits)
  float2* d;       // d.y, d.z
  float2* hit;     // t, leaf ref (bits) of the closest hit (wf_intersect -> wf_scatter)
  uint32_t* item;  // work item (| kFresh)
  uint32_t* ctr;   // rng draw counter
};
// bytes per ray position and parity: the six streams' elements
constexpr size_t kPosBytes = 2 * sizeof(float4) + 2 * sizeof(float2) + 2 * sizeof(uint32_t);

// Closest-hit lists (wf_intersect fills them, wf_scatter drains them).
// Each list holds kShards segments of medseg ray positions; the medium and
// Perlin lists share one array, the Perlin one filling its segments from the
// top (a ray is in at most one list, so together they never exceed a segment).
// Misses and emissive hits (class kListEnded) end in wf_intersect: a lane
// that finishes its traversal early ends its path while the wave's longest
// traversal runs, nearly for free. A/B on MI355X (round 4): an ended list
// drained by wf_scatter instead cost wf_scatter +19 % for wf_intersect -2.4 %,
// C3 -5 % (profiles/r04/ab/). kListEnded is a class, not a list.
enum : int32_t { kListLambertian = 0, kListGlossy = 1, kListDielectric = 2, kListMedium = 3, kListNoise = 4,
                 kListEnded = 5, kLists = 5 };
constexpr int32_t kListArrays = 4;  // Lambertian, glossy, dielectric, medium + Perlin

struct WfBufs {
  RayBuf rb[2];       // by iteration parity: wf_intersect(k) and wf_scatter(k) read rb[k & 1], wf_scatter(k) writes rb[(k + 1) & 1]
  int32_t* lists;     // 4 arrays of kShards x medseg positions: Lambertian, glossy, dielectric, medium + Perlin
  float* staging;     // [batch][npix][3] path colours
  int32_t* ctl;       // this pipe's counters, one per 256-B line (see ctl_*)
  char* spill;        // this pipe's spilled stack slots of wf_intersect (kSpillSlots rows of its grid's threads)
  int32_t* next;      // next-item counters of the work pool shards, shared by the pipes, one per 256-B line
  int32_t capacity;   // rays traced per iteration (this pipe)
  int32_t seg_cap;    // positions per continuing-ray segment
  int32_t medseg;     // positions per shard segment of a material list
  int32_t npix;       // pixels of the frame's pixel set
  int32_t sq_x, nsq;  // 8x8 pixel squares covering the pixel set: per row, total
  int32_t csamp;      // samples per chunk: a chunk is one square x csamp samples (64 * csamp items)
  int32_t batch;      // samples of the batch
  int32_t nitems;     // work items of the batch, padded to whole squares and chunks
  int32_t shard_len;  // items per pool shard (whole chunks): shard s owns [s*len, min((s+1)*len, nitems))
  int32_t s_begin;    // first sample of the batch
  FastDiv by_per, by_nsq, by_sqx;  // item decode: / (64 * csamp), / nsq, / sq_x
};

// Work items come in chunks of one 8x8 pixel square x csamp samples. Chunk c
// is square c % nsq of sample block c / nsq (so early chunks cover every
// square); item j of a chunk is pixel j % 64 of the square, sample j / 64 of
// the block. A wave's 64 fresh rays are consecutive items, so they come
// from one pixel square — the coherence the megakernel's waves get from
// their 8x8 squares. Items outside the frame or past the batch are skipped.
// it.p is the row-major pixel index (staging).
struct Item {
  int32_t srel, p, px, py;
  bool valid;
};
// Tile-listed batches (the LISTED kernels; wf_plan with a tile list): a chunk
// is one listed 64-pixel tile x csamp samples. Chunk c is virtual tile
// v = c % n_list of sample block c / n_list (WfBufs::nsq holds n_list), the
// frame tile is tiles[v], and item j of the chunk is that tile's lane j % 64
// in the frame's tile grid (the lane rule of pt_mk_plan.hpp;
// WfBufs::sq_x holds its tiles per row) — the pixels the tile id names in
// ptmi_tile_update, the listed megakernel and the listed stats resolve. An id
// outside [0, ntiles) makes the chunk's 64 lanes invalid, like items outside
// the frame.
template <bool LISTED>
struct WfList {};
template <>
struct WfList<true> {
  const int32_t* tiles;  // device, n_list ids
  int32_t ntiles;        // tiles of the frame's grid
  int32_t tw_log2;       // tile width log2 (3: 8x8, 4: 16x4, 5: 32x2, 6: 64x1)
};

__host__ __device__ __forceinline__ Item decode_item(const DevFrame& fr, const WfBufs& wb, const WfList<true>& tl,
                                                     uint32_t k) {
  Item it;
  const uint32_t per = 64u * (uint32_t)wb.csamp;
  const uint32_t c = fdiv(k, wb.by_per), j = k - c * per;
  const uint32_t blk = fdiv(c, wb.by_nsq), v = c - blk * (uint32_t)wb.nsq;  // v < n_list
  const int32_t id = tl.tiles[v];
  const bool in_grid = (uint32_t)id < (uint32_t)tl.ntiles;
  const uint32_t t = in_grid ? (uint32_t)id : 0u;  // (< 2^31: FastDiv's range)
  const int32_t ty = (int32_t)fdiv(t, wb.by_sqx), tx = (int32_t)t - ty * wb.sq_x;
  const int32_t lane = (int32_t)(j & 63u);
  const int32_t lx = tile_col0(tl.tw_log2, tx) + lane_col(tl.tw_log2, lane);
  const int32_t lr = tile_row0(tl.tw_log2, ty) + lane_row(tl.tw_log2, lane);
  it.srel = (int32_t)blk * wb.csamp + (int32_t)(j >> 6);
  it.valid = in_grid && lx < fr.w && lr < fr.n_rows && it.srel < wb.batch;
  it.p = lr * fr.w + lx;
  it.px = fr.x0 + lx;
  it.py = it.valid ? frame_row(fr, lr) : 0;
  return it;
}
__host__ __device__ __forceinline__ Item decode_item(const DevFrame& fr, const WfBufs& wb, const WfList<false>&,
                                                     uint32_t k) {
  Item it;
  // multiply-shift divisions (exact: items < 2^31, FastDiv)
  const uint32_t per = 64u * (uint32_t)wb.csamp;
  const uint32_t c = fdiv(k, wb.by_per), j = k - c * per;
  const uint32_t blk = fdiv(c, wb.by_nsq), q = c - blk * (uint32_t)wb.nsq;
  const int32_t qy = (int32_t)fdiv(q, wb.by_sqx), qx = (int32_t)q - qy * wb.sq_x;
  const int32_t lx = qx * 8 + (int32_t)(j & 7u), lr = qy * 8 + (int32_t)((j >> 3) & 7u);
  it.srel = (int32_t)blk * wb.csamp + (int32_t)(j >> 6);
  it.valid = lx < fr.w && lr < fr.n_rows && it.srel < wb.batch;
  it.p = lr * fr.w + lx;
  it.px = fr.x0 + lx;
  it.py = it.valid ? frame_row(fr, lr) : 0;
  return it;
}

// Pipes: the rays are split into PTMI_WF_PIPES independent parts, each
// driven through its own intersect/scatter loop on its own stream, so one
// pipe's kernels fill the drain at the end of another's. They share the work
// pool (next-item counters) and the staging buffer.
#ifndef PTMI_WF_PIPES
#define PTMI_WF_PIPES 4  // A/B on MI355X: 1 -> 2 pipes +15 % (C3), 2 -> 4 +5 %
#endif
constexpr int32_t kPipes = PTMI_WF_PIPES;

// Device-scope atomics are performed per cache line at the memory side, so
// counters sharing a line serialize as one: every counter gets its own
// 256-B line. Lines 0-7: next item per pool shard (shared); then per pipe:
// its status ([2]: the pool was empty after the last wf_scatter's iteration,
// written by that wf_scatter; [0], [1]: the continuing rays of the last
// wf_intersect and the [2] it saw, for the host), two sets (by
// iteration parity) of kSegs segment counts and one overflow count, and two
// sets of one count per material list and shard.
constexpr int32_t kLine = 64;
constexpr int32_t kPipeLines = 3 + 2 * kSegs + 2 * kLists * kShards;
constexpr int32_t kCtlWords = (8 + kPipeLines * kPipes) * kLine;

#ifndef PTMI_WF_CAPACITY_LOG2
// rays per iteration (all pipes). A/B: 2^21 +3 % over 2^20 (C3, mesh fog);
// with the 8-wave wf_intersect (late round 5) 2^22 over 2^21: mesh fog +5 %
// (two runs), C3 +1.6 % / +-0 (C3 varies +-1.5 %); 2^23: mesh fog +9 %, C3
// -2 % (profiles/r05/ab/ab_wf_capacity_8waves.log)
#define PTMI_WF_CAPACITY_LOG2 22
#endif
constexpr int32_t kMaxCapacity = 1 << PTMI_WF_CAPACITY_LOG2;
constexpr int32_t kSlotQuantum = kShards * kWfBlock;
constexpr size_t kSpillPipeBytes = (size_t)kSpillSlots * (PTMI_WF_MAX_BLOCKS / kPipes) * kWfBlock * 8;

static_assert((PTMI_WF_MAX_BLOCKS / kPipes) % kShards == 0, "a pipe's grid must be a multiple of the shard count");

// Work items (sample, pixel) of a batch are ids below 2^31 (FastDiv's range,
// and the kFresh bit), padded ids included: 64 per 8x8 pixel square, and the
// batch's samples rounded up to whole chunks (WfBufs::nitems); the pool
// counters may run past their shard's end by the lanes asking at once
// (< 2^24 in all). The most samples of one batch (0: no pixel).
inline int64_t wf_max_batch(const DevFrame& fr) {
  const int64_t sq_items = 64ll * ((fr.w + 7) / 8) * ((fr.n_rows + 7) / 8);
  return sq_items > 0 ? (0x7fffffffll - (1ll << 24)) / sq_items - (PTMI_WF_CHUNK_SAMPLES - 1) : 0;
}
// The same limit for a tile-listed batch, whose items are 64 per listed tile
// whatever the frame: nb <= (2^31 - 1 - 2^24) / (64 * n_list) - (chunk samples - 1).
inline int64_t wf_max_batch_listed(int32_t n_list) {
  return n_list > 0 ? (0x7fffffffll - (1ll << 24)) / (64ll * n_list) - (PTMI_WF_CHUNK_SAMPLES - 1) : 0;
}

// One batch of nb samples from s_begin in the workspace at ws: every pipe's
// buffers and work-item fields, the grids, the host loop's iteration bound
// and the workspace's size. The size depends on the frame's pixel count and
// nb only (wf_workspace_bytes).
//
// tile_list != nullptr: a tile-listed batch. Its work items cover the n_list
// listed 64-pixel tiles of the frame's tile grid (tile_grid, pt_mk_plan.hpp)
// instead of the pixel set's 8x8 squares: chunk c is virtual tile c % n_list
// of sample block c / n_list, and the kernels' LISTED decode reads the frame
// tile from tile_list (WfList above). WfBufs::nsq / by_nsq then
// hold n_list and sq_x / by_sqx the grid's tiles per row. Capacity, grids,
// shard lengths and max_iters derive from the listed items (at most
// min(npix, 64 * n_list) * nb paths are alive at once, so the ray buffers are
// never larger than the unlisted batch's); staging stays [nb][npix], so every
// region lies inside wf_workspace_bytes(fr, nb).
struct WfPlan {
  WfBufs wb[kPipes];
  unsigned grid;        // wf_intersect / wf_scatter: a multiple of kShards, so block b's shard is b % kShards
  unsigned grid_drain;  // wf_drain: one lane per continuing ray (<= capacity + the bins' padding)
  // Each item needs at most max_depth waves and every iteration advances every
  // live ray by one wave (or starts a new item), so this many iterations
  // always drain a pipe.
  int64_t max_iters;
  size_t total;
};
inline WfPlan wf_plan(const DevFrame& fr, int32_t nb, int32_t s_begin, void* ws, const int32_t* tile_list = nullptr,
                      int32_t n_list = 0) {
  WfPlan P{};
  const int32_t npix = fr.w * fr.n_rows;
  const int64_t staged = (int64_t)npix * nb;  // staging slots: [sample][frame pixel], listed or not
  int64_t items = staged;                     // paths of the batch
  if (tile_list && 64ll * n_list < npix) items = 64ll * n_list * nb;
  // rays per iteration: 2^22 (or the batch's items if fewer), whatever the
  // frame size — the pool refills the buffers, so a 4K frame needs no more
  // (the ray buffers are 56 B x 12 positions per ray: 2.8 GB at 2^22)
  int64_t cap = kMaxCapacity;
  if (items < cap) cap = items;
  cap = (cap + kPipes * kSlotQuantum - 1) / (kPipes * kSlotQuantum) * (kPipes * kSlotQuantum);
  const int32_t cp = (int32_t)(cap / kPipes);  // per pipe
  const int64_t sc = ((int64_t)cp / PTMI_WF_SEG_DIV + 63) / 64 * 64;
  const int32_t seg_cap = (int32_t)(sc < 64 ? 64 : sc);
  const size_t npos = (size_t)kSegs * seg_cap + 2 * (size_t)cp;
  // a shard's blocks take every kShards-th 128-entry chunk of wf_intersect's
  // work (<= cp + the bins' and the overflow's padding): a list segment holds them all
  const int64_t work = (int64_t)cp + 64ll * (kBins + 1);
  const int64_t chunks = (work + kWfBlock - 1) / kWfBlock;
  const int32_t medseg = (int32_t)((chunks + kShards - 1) / kShards * kWfBlock);
  // regions in workspace order: per pipe two ray buffers, per pipe the lists,
  // the shared staging, per pipe the spill rows, the counter lines
  const size_t rb_pipe = 2 * kPosBytes * npos;
  const size_t lists_pipe = kListArrays * kShards * sizeof(int32_t) * (size_t)medseg;
  const size_t lists = kPipes * rb_pipe;
  const size_t staging = (lists + kPipes * lists_pipe + 255) & ~(size_t)255;
  const size_t spill = (staging + 3 * sizeof(float) * (size_t)staged + 255) & ~(size_t)255;
  const size_t ctl = spill + kPipes * kSpillPipeBytes;
  P.total = ctl + kCtlWords * sizeof(int32_t);

  // the pixel set's 8x8 squares and the batch's chunks (in 64 bits: a size
  // query may ask for more samples than wf_max_batch allows)
  const int32_t sq_x = tile_list ? tile_grid(fr).tiles_x : (fr.w + 7) / 8;
  const int32_t nsq = tile_list ? n_list : sq_x * ((fr.n_rows + 7) / 8);
  const int32_t csamp = nb < PTMI_WF_CHUNK_SAMPLES ? nb : PTMI_WF_CHUNK_SAMPLES;
  const int64_t nchunks = csamp > 0 ? (int64_t)nsq * ((nb + csamp - 1) / csamp) : 0;
  const uintptr_t base = (uintptr_t)ws;  // integer arithmetic: a size query carves from a null base
  for (int p = 0; p < kPipes; ++p) {
    WfBufs& wb = P.wb[p];
    uintptr_t r = base + p * rb_pipe;
    auto stream = [&](size_t elem) {  // the next npos elements of the ray buffer
      const uintptr_t at = r;
      r += elem * npos;
      return at;
    };
    for (int q = 0; q < 2; ++q) {
      wb.rb[q].a = (float4*)stream(sizeof(float4));
      wb.rb[q].c = (float4*)stream(sizeof(float4));
      wb.rb[q].d = (float2*)stream(sizeof(float2));
      wb.rb[q].hit = (float2*)stream(sizeof(float2));
      wb.rb[q].item = (uint32_t*)stream(sizeof(uint32_t));
      wb.rb[q].ctr = (uint32_t*)stream(sizeof(uint32_t));
    }
    wb.lists = (int32_t*)(base + lists + p * lists_pipe);
    wb.staging = (float*)(base + staging);
    wb.next = (int32_t*)(base + ctl);
    wb.ctl = (int32_t*)(base + ctl + (8 + p * kPipeLines) * kLine * sizeof(int32_t));
    wb.spill = (char*)(base + spill + p * kSpillPipeBytes);
    wb.capacity = cp;
    wb.seg_cap = seg_cap;
    wb.medseg = medseg;
    wb.npix = npix;
    wb.sq_x = sq_x;
    wb.nsq = nsq;
    wb.batch = nb;
    wb.csamp = csamp;
    wb.nitems = (int32_t)(nchunks * 64 * csamp);
    wb.shard_len = (int32_t)((nchunks + kShards - 1) / kShards * 64 * csamp);
    wb.s_begin = s_begin;
    wb.by_per = fast_div(64u * (uint32_t)csamp);
    wb.by_nsq = fast_div((uint32_t)nsq);
    wb.by_sqx = fast_div((uint32_t)sq_x);
  }
  int64_t blocks = cp / kWfBlock;
  if (blocks > PTMI_WF_MAX_BLOCKS / kPipes) blocks = PTMI_WF_MAX_BLOCKS / kPipes;
  P.grid = (unsigned)blocks;
  P.grid_drain = (unsigned)((cp + 64 * (kBins + 1) + kWfBlock - 1) / kWfBlock);
  P.max_iters = nchunks * 64 * csamp * (int64_t)(fr.max_depth > 0 ? fr.max_depth : 1) + 2;
  return P;
}
inline size_t wf_workspace_bytes(const DevFrame& fr, int32_t batch) {
  return fr.w * fr.n_rows > 0 && batch > 0 ? wf_plan(fr, batch, 0, nullptr).total : 0;
}

}  // namespace ptmi
