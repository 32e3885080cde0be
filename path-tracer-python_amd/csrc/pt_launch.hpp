// pt_launch.hpp — host-side launchers shared between the translation units
// of libptmi.so (pt_abi.hip calls them; pt_wavefront.hip reuses the staged
// resolve of pt_megakernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "pt_device.hpp"
#include "pt_mk_plan.hpp"
#include "pt_wf_plan.hpp"

namespace ptmi {
// Where a launch's shape is decided: pt_mk_plan.hpp and pt_wf_plan.hpp (tile
// grid, workspace layouts, id limits, grids; mk_workspace_bytes, mk_max_batch,
// wf_workspace_bytes and tile_grid come from there), checked on the CPU by
// plan_check.cpp.
//
// The samples per batch of a render of s_count samples: at most max_batch (the
// integrator's id limit), halved until bytes_of_batch(batch) fits ws_bytes;
// 0 if not even one sample does.
template <class F>
int32_t fit_batch(int32_t s_count, int64_t max_batch, F&& bytes_of_batch, size_t ws_bytes) {
  int32_t batch = s_count;
  if (batch > max_batch) batch = (int32_t)max_batch;
  if (batch < 1) return 0;
  while (batch > 1 && bytes_of_batch(batch) > ws_bytes) batch = (batch + 1) / 2;
  return bytes_of_batch(batch) > ws_bytes ? 0 : batch;
}

// The one traversal dispatch of the library: (frame.traversal, stack slots
// needed = max_leaf_depth + 1) to a kernel's compile-time (STACK, TRAV),
// handed to f as two std::integral_constant<int, .> arguments. Stackless
// first; else the smallest stack rung that holds stack_needed; else, for leaf
// depth > 62, the reference's own 64-entry walk, whose stack drops pushes
// (TravRS, pt_device.hpp). FINE adds the exact 17-, 18- and 19-slot rungs
// (the staged megakernel); the direct megakernel and the wavefront use the
// coarse set and instantiate no kernel for those three.
template <bool FINE, class F>
hipError_t dispatch_traversal(const DevFrame& fr, int32_t stack_needed, F&& f) {
  using std::integral_constant;
  constexpr integral_constant<int, PTMI_TRAV_STACK> stack{};
  if (fr.traversal == PTMI_TRAV_STACKLESS)
    return f(integral_constant<int, 1>{}, integral_constant<int, PTMI_TRAV_STACKLESS>{});
  if (stack_needed <= 16) return f(integral_constant<int, 16>{}, stack);
  if constexpr (FINE) {
    if (stack_needed == 17) return f(integral_constant<int, 17>{}, stack);
    if (stack_needed == 18) return f(integral_constant<int, 18>{}, stack);
    if (stack_needed == 19) return f(integral_constant<int, 19>{}, stack);
  }
  if (stack_needed <= 20) return f(integral_constant<int, 20>{}, stack);
  if (stack_needed <= 24) return f(integral_constant<int, 24>{}, stack);
  if (stack_needed <= 32) return f(integral_constant<int, 32>{}, stack);
  if (stack_needed <= kRefStackSlots - 1) return f(integral_constant<int, 64>{}, stack);
  return f(integral_constant<int, kRefStackSlots>{}, integral_constant<int, kTravRefStack>{});
}

// Megakernel, accumulating in registers straight into accum (one work unit
// per 16x16 tile for all samples of the call).
hipError_t mk_render(const DevScene& sc, const DevFrame& fr, int32_t stack_needed, float* accum,
                     int32_t s_begin, int32_t s_count, unsigned long long* counters, hipStream_t stream);
// Megakernel over (tile, sample chunk) work units, colours staged per
// (sample, pixel) and resolved in sample order.
hipError_t mk_render_staged(const DevScene& sc, const DevFrame& fr, int32_t stack_needed, void* ws,
                            size_t ws_bytes, float* accum, int32_t s_begin, int32_t s_count,
                            unsigned long long* counters, hipStream_t stream);
// The two halves of one staged batch, for callers that schedule them
// themselves (ptmi_mk_trace_ws / ptmi_mk_trace_tiles_ws, ptmi_mk_resolve_ws):
// the megakernel into the workspace's staging, and the in-order resolve into
// accum. tile_list == nullptr: the whole frame, else the tiles of
// tile_list[0 .. n) only (device ids, ids outside the grid ignored).
hipError_t mk_trace_staged(const DevScene& sc, const DevFrame& fr, int32_t stack_needed, void* ws,
                           const int32_t* tile_list, int32_t n, int32_t s_begin, int32_t nb,
                           unsigned long long* counters, hipStream_t stream);
// stats != nullptr: every batch resolves through launch_stats_resolve.
// tile_list != nullptr (needs stats and n_list >= 1): tile-listed batches,
// which trace, stage and resolve the pixels of tile_list[0 .. n_list) only
// (device ids of the frame's tile grid, ids outside the grid ignored).
hipError_t wf_render(const DevScene& sc, const DevFrame& fr, int32_t stack_needed, void* ws, size_t ws_bytes,
                     float* accum, int32_t s_begin, int32_t s_count, unsigned long long* counters,
                     hipStream_t stream, float* stats = nullptr, const int32_t* tile_list = nullptr,
                     int32_t n_list = 0);
// Sets the wavefront tail threshold (capacity / divisor; 0 = no tail launch); returns the previous one.
int32_t wf_set_drain_at(int32_t divisor);
// accum[pixel] += staging[s][p] for s = 0..batch-1 in order (profiled as `prof_kind`).
hipError_t launch_stage_resolve(const DevFrame& fr, const float* staging, int32_t npix, int32_t batch,
                                float* accum, int prof_kind, hipStream_t stream);

// Adaptive sampling (pt_adaptive.hip; the listed trace is pt_megakernel.hip's),
// over the staged megakernel's 64-pixel tiles (tile_grid, pt_mk_plan.hpp).
// launch_stage_resolve plus the Welford update of stats[pixel] = {n, mean, M2, 0};
// tile_list == nullptr: every pixel of the frame, else the pixels of the listed tiles.
hipError_t launch_stats_resolve(const DevFrame& fr, const float* staging, int32_t npix, int32_t batch, float* accum,
                                float* stats, const int32_t* tile_list, int32_t n_tiles, int prof_kind,
                                hipStream_t stream);
// Tile errors, monotone tile states, the ascending list of active tiles and its length.
hipError_t launch_tile_update(const DevFrame& fr, const float* stats, float threshold, int32_t min_spp,
                              int32_t max_spp, int32_t* tile_state, float* tile_err, int32_t* tile_list,
                              int32_t* n_active, hipStream_t stream);
}  // namespace ptmi
