/*
 * ptmi_wf_tiles.h — the tile-listed wavefront ABI of libptmi.so: the stats
 * render of the wavefront integrator restricted to a list of the frame's
 * 64-pixel tiles, so an adaptive wavefront pass traces only the tiles still
 * above the error target. It is versioned apart from PTMI_ABI_VERSION,
 * PTMI_POST_VERSION, PTMI_GUIDE_VERSION and PTMI_TEMPORAL_VERSION: nothing in
 * ptmi.h, ptmi_post.h, ptmi_guide.h or ptmi_temporal.h changes with it. Error
 * codes, ptmi_last_error(), ptmi_scene_view, ptmi_frame, the counters, the
 * stats buffer and the tile grid (ptmi_mk_tile_grid, ptmi_tile_update) are
 * ptmi.h's; the workspace is ptmi_wf_render's (ptmi_wf_workspace_bytes).
 *
 * ---- Tiles
 *
 * A tile id t names the pixels it names everywhere else in the library
 * (ptmi_tile_update, ptmi_mk_trace_tiles_ws, ptmi_mk_resolve_stats_ws): with
 * (tile_w, tile_h, tiles_x, tiles_y) of ptmi_mk_tile_grid, tile t = ty *
 * tiles_x + tx covers local rows ty * tile_h .. and columns tx * tile_w .. of
 * the frame's pixel set, lane p of the tile being row p / tile_w, column
 * p % tile_w; lanes outside the frame are skipped. The tiles are 8x8, or
 * 16x4 / 32x2 / 64x1 on banded frames.
 *
 * ---- Work items of a listed batch
 *
 * A batch of nb samples over n listed tiles has 64 * n * nb work items, padded
 * to whole chunks of one tile x PTMI_WF_CHUNK_SAMPLES samples: chunk c is
 * virtual tile c % n of sample block c / n, and its frame tile is
 * tile_list[c % n]. Padded item ids stay below 2^31 - 2^24, so one batch holds
 * at most (2^31 - 1 - 2^24) / (64 * n) - (PTMI_WF_CHUNK_SAMPLES - 1) samples; larger calls run in
 * several batches. Everything behind the decode (the work pool, the ray
 * buffers, the material lists, the tail launch) is ptmi_wf_render's, sized
 * from the listed items, inside the same workspace.
 */
#ifndef PTMI_WF_TILES_H
#define PTMI_WF_TILES_H

#include <stddef.h>
#include <stdint.h>

#include "ptmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_WF_TILES_VERSION 1

/* ptmi_wf_render_stats restricted to the pixels of tile_list[0 .. n_tiles)
 * (int32 tile ids in device memory, distinct, as for ptmi_mk_trace_tiles_ws):
 * only those pixels are traced, staged, added to accum in sample order and
 * Welford-updated in stats, each with the path, the colour and the counter
 * contributions it has in ptmi_wf_render_stats. Every other pixel of accum and
 * stats is neither read nor written, and the staging of unlisted pixels is not
 * read. Ids outside [0, tiles_x * tiles_y) are ignored on the device. Batches
 * halve until one fits the workspace, as in ptmi_wf_render.
 *
 * n_tiles == 0 is a no-op: no launch, counters untouched. PTMI_EINVAL, each
 * with a message and before any HIP call: whatever ptmi_wf_render_stats
 * rejects in scene, frame, accum and stats (the same prologue, in the same
 * order); then n_tiles < 0 or above the grid's tile count; a NULL or
 * misaligned tile_list with n_tiles > 0; a bad sample range; a workspace
 * smaller than one sample's. Locking, stream semantics and profiling kinds are
 * ptmi_wf_render's: calls on one device are serialised, the call reads status
 * words back and is not graph-capturable. */
int ptmi_wf_render_tiles_stats(const ptmi_scene_view *scene, const ptmi_frame *frame, void *workspace,
                               size_t workspace_bytes, float *accum, float *stats,
                               const int32_t *tile_list, int32_t n_tiles,
                               int32_t sample_begin, int32_t sample_count, uint64_t *counters, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_WF_TILES_H */
