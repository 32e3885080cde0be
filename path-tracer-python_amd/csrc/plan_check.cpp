// plan_check.cpp — CPU check of the launch plans (pt_mk_plan.hpp,
// pt_wf_plan.hpp, fit_batch): a stand-alone program, no HIP runtime call, no
// GPU. `make plan_check` builds it (hipcc -x hip --cuda-host-only);
// tests/test_plan_check.py runs it. Exit 0 iff every check holds.
//
// Over a table of frames (tiny, ragged, windowed, banded, 4K) and batches it
// checks what a kernel would otherwise find out by writing out of bounds: the
// wavefront workspace's regions are aligned, disjoint and inside the
// workspace; the work-item counts respect the id limits; the megakernel's
// unit decode covers every (tile, sample, lane) exactly once and the
// wavefront's item decode every (sample, pixel); a tile-listed wavefront
// plan's regions lie inside the unlisted workspace and its decode reaches
// every (listed tile, sample, lane) once and nothing else. Three plans are
// pinned literally: the fields that set speed and that no image test sees.
// The decodes it runs are the kernels' own host/device functions (fdiv,
// frame_row, frame_index, tile_pixel, decode_item); only the
// megakernel's unit decode is restated here (locate_host).
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "pt_launch.hpp"

using namespace ptmi;

static int g_failed = 0;
static char g_ctx[160] = "";
#define PT_STR2(x) #x
#define PT_STR(x) PT_STR2(x)
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      if (++g_failed <= 40) printf("FAILED %s: %s  [%s]\n", #c, g_ctx, __FILE__ ":" PT_STR(__LINE__)); \
    }                                                                       \
  } while (0)

// A DevFrame as pt_abi.hip's to_dev_frame fills it (the fields the plans read).
static DevFrame frame(int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t band_rows = 1,
                      int32_t band_stride = 1, int32_t band_offset = 0) {
  DevFrame d{};
  d.max_depth = 50;
  d.width = width, d.height = height, d.x0 = x0, d.y0 = y0, d.w = w, d.h = h;
  d.band_rows = band_rows, d.band_stride = band_stride, d.band_offset = band_offset;
  for (int32_t r = 0; r < h; ++r)
    if ((r / band_rows) % band_stride == band_offset) ++d.n_rows;
  return d;
}

struct Case {
  const char* name;
  DevFrame fr;
};
static std::vector<Case> frames() {
  return {
      {"1x1", frame(1, 1, 0, 0, 1, 1)},
      {"3x1", frame(3, 1, 0, 0, 3, 1)},
      {"13x7", frame(13, 7, 0, 0, 13, 7)},
      {"64x64", frame(64, 64, 0, 0, 64, 64)},
      {"800x800", frame(800, 800, 0, 0, 800, 800)},
      {"800x800 window 397,301 5x3", frame(800, 800, 397, 301, 5, 3)},
      {"800x800 band 4/8/3", frame(800, 800, 0, 0, 800, 800, 4, 8, 3)},
      {"800x800 band 2/4/1", frame(800, 800, 0, 0, 800, 800, 2, 4, 1)},
      {"800x800 band 1/8/0", frame(800, 800, 0, 0, 800, 800, 1, 8, 0)},
      {"800x800 band 8/3/2", frame(800, 800, 0, 0, 800, 800, 8, 3, 2)},
      {"3840x2160", frame(3840, 2160, 0, 0, 3840, 2160)},
  };
}

// DevFrame::n_rows against the kernels' frame_row: strictly increasing image
// rows of the window, each in a band with the frame's offset, and -1 from
// n_rows on.
static void check_frame(const DevFrame& fr) {
  int32_t prev = -1;
  for (int32_t lr = 0; lr < fr.n_rows; ++lr) {
    const int32_t row = frame_row(fr, lr);
    CHECK(row > prev && row >= fr.y0 && row < fr.y0 + fr.h);
    CHECK(((row - fr.y0) / fr.band_rows) % fr.band_stride == fr.band_offset);
    prev = row;
  }
  for (int32_t lr = fr.n_rows; lr < fr.n_rows + 3 * fr.band_rows; ++lr) CHECK(frame_row(fr, lr) == -1);
}

// A workspace address that is never dereferenced.
static char* const kBase = (char*)(uintptr_t)0x7000000000ull;
constexpr int kPerCu = 20, kNcu = 256;  // vol2's occupancy on a 256-CU MI355X

// ------------------------------------------------------------------ tile grid
static void check_tile_grid(const DevFrame& fr) {
  const TileGrid g = tile_grid(fr);
  const int32_t tw = 1 << g.tw_log2, th = 64 >> g.tw_log2;
  CHECK(g.tw_log2 >= 3 && g.tw_log2 <= 6);
  CHECK(g.tiles_x == (fr.w + tw - 1) / tw);
  CHECK(g.ntiles == g.tiles_x * ((fr.n_rows + th - 1) / th));
  // a banded frame's tile never straddles two bands
  if (fr.band_stride > 1) CHECK(fr.band_rows % th == 0 || th == 1);
  if (fr.band_stride <= 1) CHECK(th == 8);
  // every pixel of the frame is lane p of exactly one tile (the kernels' tile_pixel, pt_mk_plan.hpp)
  if ((int64_t)fr.w * fr.n_rows <= (1 << 20)) {
    std::vector<uint8_t> seen((size_t)fr.w * fr.n_rows, 0);
    for (int32_t t = 0; t < g.ntiles; ++t)
      for (int32_t p = 0; p < 64; ++p) {
        int32_t col, lr;
        if (!tile_pixel(fr, g, t, p, col, lr)) continue;
        CHECK(col >= 0 && lr >= 0 && col / tw == t % g.tiles_x && lr / th == t / g.tiles_x && col % tw + (lr % th) * tw == p);
        ++seen[(size_t)lr * fr.w + col];
      }
    CHECK(std::all_of(seen.begin(), seen.end(), [](uint8_t c) { return c == 1; }));
  }
}

// ------------------------------------------------------------------ megakernel
// COPY of the persistent branch of locate() of mk_render_kernel
// (pt_megakernel.hip), the one decode still restated here: as a host/device
// function it compiled to other device code in the unlisted staged kernels
// (DESIGN.md §3), so it stays in its kernel. Its pieces (fdiv, tile_col0,
// tile_row0) are the kernel's own. A unit is item >> 6.
struct Unit {
  int32_t col, row, s;  // tile origin (window column, local row), sample of the batch
};
static Unit locate_host(const DevFrame& fr, const MkWork& wk, uint32_t v, const std::vector<int32_t>* list) {
  const uint32_t sh = fdiv(v, wk.by_len), j = v - sh * (uint32_t)wk.shard_len;
  const uint32_t tq = fdiv(j, wk.by_nb);
  uint32_t t = tq * (uint32_t)kMkShards + sh;
  const int32_t s = (int32_t)(j - tq * (uint32_t)wk.nb);
  if (list) {
    const uint32_t id = t < (uint32_t)wk.n_list ? (uint32_t)(*list)[t] : 0xffffffffu;
    if (id >= (uint32_t)wk.ntiles) return Unit{0, fr.n_rows, s};
    t = id;
  }
  const uint32_t ty = fdiv(t, wk.by_tiles_x);
  return Unit{tile_col0(wk.tw_log2, (int32_t)(t - ty * (uint32_t)wk.tiles_x)), tile_row0(wk.tw_log2, (int32_t)ty), s};
}

// Every (tile, sample) of the launch is exactly one unit, every other unit
// lies outside the frame; with check_tile_grid's lanes that is every (tile,
// sample, lane) exactly once. Launches of more than 2^23 units are checked
// at every 4099th unit and around every shard's ends against plain division.
static void check_mk_cover(const DevFrame& fr, const MkWork& wk, const std::vector<int32_t>* list) {
  const TileGrid g = tile_grid(fr);
  const int32_t tw = 1 << g.tw_log2, th = 64 >> g.tw_log2;
  auto tile_of = [&](const Unit& u) -> int64_t {  // -1: outside the frame
    if (u.row >= fr.n_rows || u.col >= fr.w) return -1;
    CHECK(u.col % tw == 0 && u.row % th == 0);
    return (int64_t)(u.row / th) * g.tiles_x + u.col / tw;
  };
  auto expect = [&](uint32_t v) {  // the decode by plain division
    const uint32_t sh = v / (uint32_t)wk.shard_len, j = v % (uint32_t)wk.shard_len;
    int64_t t = (int64_t)(j / (uint32_t)wk.nb) * kMkShards + sh;
    if (list) t = t < wk.n_list && (uint32_t)(*list)[t] < (uint32_t)wk.ntiles ? (*list)[t] : -1;
    if (t >= wk.ntiles) t = -1;
    return std::pair<int64_t, int32_t>(t, (int32_t)(j % (uint32_t)wk.nb));
  };
  if (wk.nunits > (1 << 23)) {
    auto at = [&](int64_t v) {
      if (v < 0 || v >= wk.nunits) return;
      const Unit u = locate_host(fr, wk, (uint32_t)v, list);
      const auto e = expect((uint32_t)v);
      CHECK(tile_of(u) == e.first && u.s == e.second);
    };
    for (int64_t v = 0; v < wk.nunits; v += 4099) at(v);
    for (int sh = 0; sh <= kMkShards; ++sh)
      for (int64_t d = -64; d < 64; ++d) at((int64_t)sh * wk.shard_len + d);
    return;
  }
  std::vector<uint8_t> seen((size_t)wk.ntiles * wk.nb, 0);
  for (uint32_t v = 0; v < (uint32_t)wk.nunits; ++v) {
    const Unit u = locate_host(fr, wk, v, list);
    CHECK(u.s >= 0 && u.s < wk.nb);
    const int64_t t = tile_of(u);
    if (t >= 0) ++seen[(size_t)t * wk.nb + u.s];
  }
  std::vector<uint8_t> want((size_t)wk.ntiles * wk.nb, list ? 0 : 1);
  if (list)
    for (int32_t k = 0; k < wk.n_list; ++k)
      if ((uint32_t)(*list)[k] < (uint32_t)wk.ntiles)
        for (int32_t s = 0; s < wk.nb; ++s) ++want[(size_t)(*list)[k] * wk.nb + s];
  CHECK(seen == want);
}

static void check_mk(const DevFrame& fr, int32_t nb, const std::vector<int32_t>* list) {
  const int32_t npix = fr.w * fr.n_rows;
  const int32_t n_list = list ? (int32_t)list->size() : 0;
  const MkPlan P = mk_plan(fr, kBase, nb, list ? list->data() : nullptr, n_list, kPerCu, kNcu);
  CHECK(P.err == hipSuccess);
  if (P.err != hipSuccess) return;
  const MkWork& wk = P.wk;
  const MkWorkspace w = mk_workspace(npix, nb);
  const size_t raw = 3 * sizeof(float) * (size_t)npix * (size_t)nb;
  CHECK(w.staging >= raw && w.staging < raw + 256 && w.staging % 256 == 0);
  CHECK((char*)wk.ctl == kBase + w.staging);  // directly after staging, 256-B aligned
  CHECK((uintptr_t)wk.ctl % 256 == 0);
  CHECK(P.ctl_bytes == (size_t)kMkShards * kMkCtlLine * sizeof(int32_t));
  CHECK(w.staging + P.ctl_bytes == mk_workspace_bytes(npix, nb));
  CHECK(wk.nunits == wk.shard_len * kMkShards);
  CHECK(wk.nb == nb && wk.nunits % nb == 0);
  CHECK((int64_t)wk.nunits * 64 < (1ll << 32));
  CHECK((int64_t)wk.nunits >= (list ? (int64_t)n_list : (int64_t)tile_grid(fr).ntiles) * nb);
  CHECK(P.waves >= 1 && P.waves <= (unsigned)wk.nunits);
  CHECK(wk.tail_div >= 1);
  CHECK(wk.csamp == PTMI_MK_CHUNK_SAMPLES);
  CHECK(wk.ntiles == tile_grid(fr).ntiles && wk.tiles_x == tile_grid(fr).tiles_x && wk.tw_log2 == tile_grid(fr).tw_log2);
  CHECK(wk.n_list == n_list);
  check_mk_cover(fr, wk, list);
}

// ------------------------------------------------------------------ wavefront
struct Region {
  uintptr_t lo, hi;
  const char* what;
};

// The staging slot srel * npix + p of work item k as the kernels' decode_item
// (pt_wf_plan.hpp) gives it, or -1 for an item outside the frame or past the
// batch. A valid item's image pixel is what plain arithmetic gives for its
// (local row, window column), and both frame_index overloads agree.
static int64_t wf_slot(const DevFrame& fr, const WfBufs& wb, const Item& it) {
  if (!it.valid) return -1;
  const int32_t lr = it.p / fr.w, col = it.p % fr.w;
  CHECK(it.px == fr.x0 + col && it.py == frame_row(fr, lr) && it.py >= fr.y0 && it.py < fr.y0 + fr.h);
  const size_t pix = (size_t)it.py * (size_t)fr.width + (size_t)it.px;
  CHECK(frame_index(fr, lr, col) == pix && frame_index(fr, it.p) == pix);
  return (int64_t)it.srel * wb.npix + it.p;
}

// Every (sample, pixel) of the batch is exactly one work item, so every
// staging slot is written once and none outside staging. Batches of more
// than 2^23 items are checked at every 4099th item against plain division.
static void check_wf_cover(const DevFrame& fr, const WfBufs& wb) {
  if (wb.nitems > (1 << 23)) {
    for (uint32_t k = 0; k < (uint32_t)wb.nitems; k += 4099) {
      const uint32_t per = 64u * (uint32_t)wb.csamp, c = k / per, j = k % per, q = c % (uint32_t)wb.nsq;
      const int32_t lx = (int32_t)(q % (uint32_t)wb.sq_x) * 8 + (int32_t)(j & 7u);
      const int32_t lr = (int32_t)(q / (uint32_t)wb.sq_x) * 8 + (int32_t)((j >> 3) & 7u);
      const int32_t srel = (int32_t)(c / (uint32_t)wb.nsq) * wb.csamp + (int32_t)(j >> 6);
      const bool in = lx < fr.w && lr < fr.n_rows && srel < wb.batch;
      CHECK(wf_slot(fr, wb, decode_item(fr, wb, WfList<false>{}, k)) == (in ? (int64_t)srel * wb.npix + (lr * fr.w + lx) : -1));
    }
    return;
  }
  std::vector<uint8_t> seen((size_t)wb.npix * wb.batch, 0);
  for (uint32_t k = 0; k < (uint32_t)wb.nitems; ++k) {
    const int64_t slot = wf_slot(fr, wb, decode_item(fr, wb, WfList<false>{}, k));
    CHECK(slot < (int64_t)seen.size());
    if (slot >= 0 && slot < (int64_t)seen.size()) ++seen[(size_t)slot];
  }
  CHECK(std::all_of(seen.begin(), seen.end(), [](uint8_t c) { return c == 1; }));
}

// The same through the LISTED decode_item. -2: the plan's nsq exceeds the
// list, so the device would read past it (never: nsq is n_list). The guard
// compares nsq's range with list.size() by plain division before the call; it
// does not look at the decode's own v.
static int64_t wf_listed_slot(const DevFrame& fr, const WfBufs& wb, const std::vector<int32_t>& list,
                              const TileGrid& g, uint32_t k) {
  if ((k / (64u * (uint32_t)wb.csamp)) % (uint32_t)wb.nsq >= list.size()) return -2;
  return wf_slot(fr, wb, decode_item(fr, wb, WfList<true>{list.data(), g.ntiles, g.tw_log2}, k));
}

// The listed decode reaches every (listed tile, sample, lane) inside the frame
// exactly once (the ids are distinct) and no other staging slot. Batches of
// more than 2^23 items, or whose staging has more than 2^26 slots, are
// checked at every 4099th item against plain division.
static void check_wf_listed_cover(const DevFrame& fr, const WfBufs& wb, const std::vector<int32_t>& list) {
  const TileGrid g = tile_grid(fr);
  const int32_t tw = 1 << g.tw_log2, th = 64 >> g.tw_log2;
  auto plain = [&](uint32_t k) -> int64_t {
    const uint32_t per = 64u * (uint32_t)wb.csamp, c = k / per, j = k % per;
    const int32_t id = list[c % (uint32_t)list.size()];
    const int32_t srel = (int32_t)(c / (uint32_t)list.size()) * wb.csamp + (int32_t)(j / 64u);
    if (id < 0 || id >= g.ntiles) return -1;
    const int32_t lx = (id % g.tiles_x) * tw + (int32_t)(j % 64u) % tw, lr = (id / g.tiles_x) * th + (int32_t)(j % 64u) / tw;
    return lx < fr.w && lr < fr.n_rows && srel < wb.batch ? (int64_t)srel * wb.npix + ((int64_t)lr * fr.w + lx) : -1;
  };
  if (wb.nitems > (1 << 23) || (int64_t)wb.npix * wb.batch > (1ll << 26)) {
    for (uint32_t k = 0; k < (uint32_t)wb.nitems; k += 4099) CHECK(wf_listed_slot(fr, wb, list, g, k) == plain(k));
    for (int64_t k = (int64_t)wb.nitems - 64; k < wb.nitems; ++k)
      if (k >= 0) CHECK(wf_listed_slot(fr, wb, list, g, (uint32_t)k) == plain((uint32_t)k));
    return;
  }
  std::vector<uint8_t> seen((size_t)wb.npix * wb.batch, 0), want(seen.size(), 0);
  for (uint32_t k = 0; k < (uint32_t)wb.nitems; ++k) {
    const int64_t slot = wf_listed_slot(fr, wb, list, g, k);
    CHECK(slot >= -1 && slot < (int64_t)seen.size());
    if (slot >= 0 && slot < (int64_t)seen.size()) ++seen[(size_t)slot];
  }
  for (int32_t id : list) {
    if (id < 0 || id >= g.ntiles) continue;
    for (int32_t p = 0; p < 64; ++p) {
      const int32_t lx = (id % g.tiles_x) * tw + p % tw, lr = (id / g.tiles_x) * th + p / tw;
      if (lx < fr.w && lr < fr.n_rows)
        for (int32_t s = 0; s < wb.batch; ++s) ++want[(size_t)s * wb.npix + ((size_t)lr * fr.w + lx)];
    }
  }
  CHECK(seen == want);
}

// list != nullptr: the tile-listed plan of the same frame and batch.
static void check_wf(const DevFrame& fr, int32_t nb, const std::vector<int32_t>* list = nullptr) {
  const int32_t npix = fr.w * fr.n_rows;
  const int32_t n_list = list ? (int32_t)list->size() : 0;
  const WfPlan P = wf_plan(fr, nb, 7, kBase, list ? list->data() : nullptr, n_list);
  // a listed plan lies inside the unlisted workspace, whose size does not change
  if (list) CHECK(P.total <= wf_workspace_bytes(fr, nb));
  else CHECK(P.total == wf_workspace_bytes(fr, nb));
  const uintptr_t base = (uintptr_t)kBase, end = base + P.total;
  const WfBufs& w0 = P.wb[0];
  std::vector<Region> R;
  auto add = [&](const void* p, size_t bytes, const char* what) {
    R.push_back(Region{(uintptr_t)p, (uintptr_t)p + bytes, what});
  };
  for (int p = 0; p < kPipes; ++p) {
    const WfBufs& wb = P.wb[p];
    const size_t npos = (size_t)kSegs * wb.seg_cap + 2 * (size_t)wb.capacity;  // segments, overflow, fresh rays
    for (int q = 0; q < 2; ++q) {
      add(wb.rb[q].a, sizeof(float4) * npos, "rb.a");
      add(wb.rb[q].c, sizeof(float4) * npos, "rb.c");
      add(wb.rb[q].d, sizeof(float2) * npos, "rb.d");
      add(wb.rb[q].hit, sizeof(float2) * npos, "rb.hit");
      add(wb.rb[q].item, sizeof(uint32_t) * npos, "rb.item");
      add(wb.rb[q].ctr, sizeof(uint32_t) * npos, "rb.ctr");
    }
    add(wb.lists, sizeof(int32_t) * kListArrays * kShards * (size_t)wb.medseg, "lists");
    add(wb.spill, kSpillPipeBytes, "spill");
    add(wb.ctl, sizeof(int32_t) * kPipeLines * kLine, "ctl");
    CHECK((uintptr_t)wb.ctl % 256 == 0);
    // the spill rows hold kSpillSlots 8-byte slots of every thread of the grid
    CHECK((size_t)kSpillSlots * P.grid * kWfBlock * 8 <= kSpillPipeBytes);
    // shared by the pipes: staging, the pool counters, every item field
    CHECK(wb.staging == w0.staging && wb.next == w0.next);
    CHECK(wb.capacity == w0.capacity && wb.seg_cap == w0.seg_cap && wb.medseg == w0.medseg && wb.npix == npix);
    CHECK(wb.sq_x == w0.sq_x && wb.nsq == w0.nsq && wb.csamp == w0.csamp && wb.batch == nb);
    CHECK(wb.nitems == w0.nitems && wb.shard_len == w0.shard_len && wb.s_begin == 7);
    CHECK(wb.by_per.d == 64u * (uint32_t)wb.csamp && wb.by_nsq.d == (uint32_t)wb.nsq && wb.by_sqx.d == (uint32_t)wb.sq_x);
  }
  add(w0.staging, 3 * sizeof(float) * (size_t)npix * (size_t)nb, "staging");
  add(w0.next, sizeof(int32_t) * 8 * kLine, "next");
  CHECK((uintptr_t)w0.next % 256 == 0);
  std::sort(R.begin(), R.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
  for (size_t i = 0; i < R.size(); ++i) {
    CHECK(R[i].lo % 16 == 0);
    CHECK(R[i].lo >= base && R[i].hi <= end && R[i].lo < R[i].hi);
    if (i + 1 < R.size()) CHECK(R[i].hi <= R[i + 1].lo);  // sorted: pairwise disjoint
  }
  CHECK(R.back().hi == end);  // the counter lines close the workspace
  // the memset before a batch zeroes the pool counters and every pipe's lines
  CHECK((uintptr_t)w0.next + kCtlWords * sizeof(int32_t) == end);

  if (list) {
    CHECK(w0.sq_x == tile_grid(fr).tiles_x && w0.nsq == n_list);
    // no more rays in flight than the listed paths, nor than the unlisted batch's
    CHECK(w0.capacity <= wf_plan(fr, nb, 7, kBase).wb[0].capacity);
    CHECK((int64_t)nb <= wf_max_batch_listed(n_list));
  } else {
    CHECK(w0.sq_x == (fr.w + 7) / 8 && w0.nsq == w0.sq_x * ((fr.n_rows + 7) / 8));
  }
  CHECK(w0.csamp >= 1 && w0.csamp <= PTMI_WF_CHUNK_SAMPLES && w0.csamp <= nb);
  CHECK(w0.nitems > 0 && w0.nitems % (64 * w0.csamp) == 0);
  CHECK((int64_t)w0.nitems >= 64ll * w0.nsq * nb);  // every (square, sample, lane) has an id
  CHECK((int64_t)w0.nitems + (1ll << 24) <= (1ll << 31));
  CHECK(w0.shard_len % (64 * w0.csamp) == 0 && (int64_t)w0.shard_len * kShards >= w0.nitems);
  CHECK((int64_t)w0.shard_len * (kShards - 1) < w0.nitems + 64 * w0.csamp * (kShards - 1));
  // a list segment holds a shard's share of wf_intersect's work, in whole blocks
  const int64_t work = (int64_t)w0.capacity + 64 * (kBins + 1);
  const int64_t share = ((work + kWfBlock - 1) / kWfBlock + kShards - 1) / kShards * kWfBlock;
  CHECK(w0.medseg >= share && (int64_t)w0.medseg * kShards >= work);
  CHECK(w0.capacity % kSlotQuantum == 0 && (int64_t)w0.capacity * kPipes <= kMaxCapacity);
  CHECK(w0.seg_cap >= 64 && w0.seg_cap % 64 == 0 && (int64_t)w0.seg_cap * PTMI_WF_SEG_DIV >= w0.capacity);
  // block b's shard is b % kShards; one lane per ray of an iteration
  CHECK(P.grid >= (unsigned)kShards && P.grid % kShards == 0 && P.grid <= PTMI_WF_MAX_BLOCKS / kPipes);
  CHECK((int64_t)P.grid * kWfBlock <= w0.capacity);
  CHECK((int64_t)P.grid_drain * kWfBlock >= work);
  CHECK(P.max_iters == (int64_t)w0.nitems * fr.max_depth + 2);
  if (list) check_wf_listed_cover(fr, w0, *list);
  else check_wf_cover(fr, w0);
}

// ------------------------------------------------------------------ literal plans
static void check_literals() {
  const DevFrame whole = frame(800, 800, 0, 0, 800, 800), band = frame(800, 800, 0, 0, 800, 800, 4, 8, 3);
  {
    snprintf(g_ctx, sizeof g_ctx, "literal: 800x800 whole, nb 64");
    const MkPlan P = mk_plan(whole, kBase, 64, nullptr, 0, 20, 256);
    CHECK(P.err == hipSuccess && P.wk.tw_log2 == 3 && P.wk.tiles_x == 100 && P.wk.shard_len == 80000);
    CHECK(P.wk.nunits == 640000 && P.waves == 5120 && P.wk.tail_div == 2560 && P.wk.csamp == 32);
  }
  {
    snprintf(g_ctx, sizeof g_ctx, "literal: 800x800 band 4/8/3, nb 64 (small grid, small-batch tail)");
    const MkPlan P = mk_plan(band, kBase, 64, nullptr, 0, 20, 256);
    CHECK(P.err == hipSuccess && P.wk.tw_log2 == 4 && P.wk.tiles_x == 50 && P.wk.shard_len == 10048);
    CHECK(P.wk.nunits == 80384 && P.waves == 2560 && P.wk.tail_div == 640);
    CHECK(mk_max_batch(band) == 53430 && wf_workspace_bytes(band, 64) == 2989347840ull);
  }
  {
    snprintf(g_ctx, sizeof g_ctx, "literal: 800x800 whole, 100 listed tiles, nb 16");
    std::vector<int32_t> list(100);
    for (int k = 0; k < 100; ++k) list[k] = 97 * k;
    const MkPlan P = mk_plan(whole, kBase, 16, list.data(), 100, 20, 256);
    CHECK(P.err == hipSuccess && P.wk.shard_len == 208 && P.wk.nunits == 1664 && P.waves == 1664);
    CHECK(P.wk.tail_div == 416 && P.wk.ntiles == 10000 && P.wk.n_list == 100);
  }
  snprintf(g_ctx, sizeof g_ctx, "fit_batch");
  auto bytes = [](int32_t b) { return (size_t)b * 100; };
  CHECK(fit_batch(10, 4, bytes, 1000) == 4 && fit_batch(3, 4, bytes, 1000) == 3);
  CHECK(fit_batch(10, 100, bytes, 250) == 2);  // 10 -> 5 -> 3 -> 2
  CHECK(fit_batch(10, 100, bytes, 100) == 1 && fit_batch(10, 100, bytes, 99) == 0);
  CHECK(fit_batch(10, 0, bytes, 1000) == 0 && fit_batch(0, 4, bytes, 1000) == 0);
}

int main() {
  const int32_t batches[] = {1, 2, 3, 4, 5, 16, 64, 1024};
  int plans = 0;
  for (const Case& c : frames()) {
    const DevFrame& fr = c.fr;
    snprintf(g_ctx, sizeof g_ctx, "%s: frame rows and pixels", c.name);
    check_frame(fr);
    snprintf(g_ctx, sizeof g_ctx, "%s: tile grid", c.name);
    check_tile_grid(fr);
    const int64_t mk_max = mk_max_batch(fr), wf_max = wf_max_batch(fr);
    CHECK(mk_max >= 1 && mk_max <= 0x7fffffff && wf_max >= 1);
    std::vector<int32_t> nbs(std::begin(batches), std::end(batches));
    nbs.push_back((int32_t)mk_max);
    for (int32_t nb : nbs) {
      if (nb <= mk_max) {
        snprintf(g_ctx, sizeof g_ctx, "%s: megakernel, batch %d", c.name, nb);
        check_mk(fr, nb, nullptr);
        ++plans;
      }
      // wf_render plans no batch above wf_max_batch: the limit itself stands in
      const int32_t wnb = (int32_t)std::min<int64_t>(nb, wf_max);
      snprintf(g_ctx, sizeof g_ctx, "%s: wavefront, batch %d", c.name, wnb);
      check_wf(fr, wnb);
      ++plans;
    }
    snprintf(g_ctx, sizeof g_ctx, "%s: wavefront, batch wf_max_batch %lld", c.name, (long long)wf_max);
    check_wf(fr, (int32_t)wf_max);
    snprintf(g_ctx, sizeof g_ctx, "%s: megakernel id limit %lld", c.name, (long long)mk_max);
    CHECK(mk_plan(fr, kBase, (int32_t)mk_max, nullptr, 0, kPerCu, kNcu).err == hipSuccess);
    CHECK(mk_plan(fr, kBase, (int32_t)mk_max + 1, nullptr, 0, kPerCu, kNcu).err == hipErrorInvalidValue);
    CHECK(mk_plan(fr, kBase, 0, nullptr, 0, kPerCu, kNcu).err == hipErrorInvalidValue);
    // listed launches: every third tile, then ids outside the grid (ignored)
    const int32_t ntiles = tile_grid(fr).ntiles;
    std::vector<int32_t> list;
    for (int32_t t = 0; t < ntiles; t += 3) list.push_back(t);
    if (list.size() + 2 <= (size_t)ntiles) {
      list.push_back(ntiles);
      list.push_back(-1);
    }
    for (int32_t nb : {1, 3, 16}) {
      snprintf(g_ctx, sizeof g_ctx, "%s: megakernel, %zu listed tiles, batch %d", c.name, list.size(), nb);
      check_mk(fr, nb, &list);
      ++plans;
    }
  }
  // tile-listed wavefront plans: n_list in {1, 5, 8, 9, ntiles} tiles spread
  // over the grid, the last tile (an edge tile) among them and, from 5 ids on,
  // one id outside the grid; then the listed id limit
  for (const Case& c : frames()) {
    const DevFrame& fr = c.fr;
    const int32_t ntiles = tile_grid(fr).ntiles;
    int32_t last = 0;
    for (int32_t want : {1, 5, 8, 9, ntiles}) {
      const int32_t n_list = std::min(want, ntiles);
      if (n_list == last) continue;
      last = n_list;
      std::vector<int32_t> list(n_list);
      for (int32_t k = 0; k < n_list; ++k) list[k] = (int32_t)((int64_t)k * ntiles / n_list);
      list[n_list - 1] = ntiles - 1;
      if (n_list >= 5 && n_list < ntiles) list[2] = ntiles;
      for (int32_t nb : {1, 3, 5, 16}) {
        snprintf(g_ctx, sizeof g_ctx, "%s: wavefront, %d listed tiles, batch %d", c.name, n_list, nb);
        check_wf(fr, nb, &list);
        ++plans;
      }
      const int64_t lmax = wf_max_batch_listed(n_list);
      snprintf(g_ctx, sizeof g_ctx, "%s: wavefront, %d listed tiles, id limit %lld", c.name, n_list, (long long)lmax);
      CHECK(lmax >= 1);
      check_wf(fr, (int32_t)lmax, &list);  // (checks nitems + 2^24 <= 2^31)
      ++plans;
    }
  }
  check_literals();
  if (g_failed) {
    printf("plan_check: %d checks FAILED\n", g_failed);
    return 1;
  }
  printf("plan_check: %d plans ok\n", plans);
  return 0;
}
