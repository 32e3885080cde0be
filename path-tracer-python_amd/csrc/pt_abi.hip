// pt_abi.hip — the extern "C" boundary of libptmi.so (declared in
// include/ptmi.h): argument validation, scene/frame conversion, launch of the
// megakernel / wavefront / tone-map / clear kernels. No device allocation
// happens inside a render call; the megakernel calls are asynchronous and
// graph-capturable, the wavefront reads its live-slot counts back every 4
// iterations (pinned 4-byte slots, allocated once).
// Layout: the four small kernels; conversion of scene and frame; the shared
// argument checks; one body per pair of entry points that differ by an
// optional argument (plain / stats render, whole-frame / listed trace, plain /
// stats resolve, the clears, the tone maps); the extern "C" entry points.
// Every rejected argument and every no-op returns before the first HIP call.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/ptmi_wf_tiles.h"
#include "pt_args.hpp"
#include "pt_image.hpp"
#include "pt_launch.hpp"
#include "pt_prof.hpp"

namespace ptmi {

// clear_accum_buffer, kernels.py:1205-1209 (restricted to the frame's pixel set).
__global__ __launch_bounds__(kBlock) void clear_kernel(DevFrame fr, float* __restrict__ accum) {
  const int32_t npix = fr.w * fr.n_rows;
  for (int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x); i < npix; i += (int32_t)(gridDim.x * kBlock)) {
    float* p = accum + 3 * frame_index(fr, i);
    p[0] = 0.0f;
    p[1] = 0.0f;
    p[2] = 0.0f;
  }
}

// LivePreview.buffer_to_image, preview.py:117-132. numpy evaluates
// accum * scale in f32 (NEP 50), sqrt(max(0, x)) in f32, * 255.999 in f32,
// clip to [0, 255] and truncates to u8.
__global__ __launch_bounds__(kBlock) void tonemap_kernel(const float* __restrict__ accum, uint8_t* __restrict__ out,
                                                         int32_t n, float scale) {
  for (int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x); i < n; i += (int32_t)(gridDim.x * kBlock)) {
    float x = accum[i] * scale;
    float g = sqrtf(pt_maxf(x, 0.0f));
    float v = g * 255.999f;
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    out[i] = (uint8_t)(int32_t)v;
  }
}

// clear_kernel for the stats buffer: {n, mean, M2, reserved} = 0 on the frame's pixel set.
__global__ __launch_bounds__(kBlock) void stats_clear_kernel(DevFrame fr, float4* __restrict__ stats) {
  const int32_t npix = fr.w * fr.n_rows;
  for (int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x); i < npix; i += (int32_t)(gridDim.x * kBlock)) {
    stats[frame_index(fr, i)] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// tonemap_kernel with the scale of each pixel's own sample count n =
// stats[pixel][0]: scale = (float)(1.0 / (double)max(n, 1)). With one n for
// the whole image this is tonemap_kernel bit for bit.
__global__ __launch_bounds__(kBlock) void tonemap_stats_kernel(const float* __restrict__ accum,
                                                               const float4* __restrict__ stats,
                                                               uint8_t* __restrict__ out, int32_t n) {
  for (int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x); i < n; i += (int32_t)(gridDim.x * kBlock)) {
    const float cnt = stats[i / 3].x;
    const float scale = (float)(1.0 / (double)(cnt > 1.0f ? cnt : 1.0f));
    float x = accum[i] * scale;
    float g = sqrtf(pt_maxf(x, 0.0f));
    float v = g * 255.999f;
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    out[i] = (uint8_t)(int32_t)v;
  }
}
}  // namespace ptmi

using namespace ptmi;

static thread_local std::string g_err;

// pt_args.hpp: one slot for the entry points of every translation unit.
int ptmi::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

static int check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) return fail(PTMI_EHIP, "%s: %s", what, hipGetErrorString(e));
  return PTMI_OK;
}

static int to_dev_scene(const ptmi_scene_view* s, DevScene& d) {
  if (!s) return fail(PTMI_EINVAL, "scene is NULL");
  int32_t np = s->num_spheres + s->num_quads + s->num_triangles;
  if (s->num_spheres < 0 || s->num_quads < 0 || s->num_triangles < 0 || s->n_inner < 0)
    return fail(PTMI_EINVAL, "negative scene counts");
  if (np > 0x0fffffff) return fail(PTMI_ECAPACITY, "too many primitives (%d)", np);
  if (s->num_spheres > (1 << 25) || s->num_quads > (1 << 25) || s->num_triangles > (1 << 25))
    return fail(PTMI_ECAPACITY, "more than 2^25 primitives of one type (25-bit leaf index)");
  if (np > 0 && s->n_inner != np - 1)
    return fail(PTMI_EINVAL, "binary BVH with one primitive per leaf needs n_inner = prims - 1 (%d vs %d)",
                s->n_inner, np - 1);
  if (s->n_inner > 0 && bad16(s->nodes)) return fail(PTMI_EINVAL, "nodes NULL/misaligned");
  if (s->num_spheres > 0 && bad16(s->spheres)) return fail(PTMI_EINVAL, "spheres");
  if (s->num_quads > 0 && bad16(s->quads)) return fail(PTMI_EINVAL, "quads");
  if (s->num_triangles > 0 && bad16(s->tris)) return fail(PTMI_EINVAL, "tris");
  if (np > 0 && bad16(s->mats)) return fail(PTMI_EINVAL, "mats");
  if (bad16(s->perlin_vec) || !s->perlin_perm) return fail(PTMI_EINVAL, "perlin tables");
  if (s->num_images < 0 || s->num_images > PTMI_MAX_IMAGES) return fail(PTMI_EINVAL, "num_images");
  if (s->num_images > 0 && !s->texels) return fail(PTMI_EINVAL, "texels");
  // The reference's 64-slot stack never overflows for leaf depth <= 62
  // (kernels.py:719-740); deeper BVHs run its exact walk on its own nodes,
  // silent drops included (TravRS, pt_device.hpp), which needs ref_nodes.
  if (s->max_leaf_depth < 0) return fail(PTMI_EINVAL, "negative max_leaf_depth");
  if (s->max_leaf_depth > 62 && np > 0 && !s->ref_nodes)
    return fail(PTMI_EINVAL, "BVH leaf depth %d > 62 needs ref_nodes (the reference's 64-entry stack walk)",
                s->max_leaf_depth);
  if (s->num_bvh_nodes != (np > 0 ? 2 * np - 1 : 0))
    return fail(PTMI_EINVAL, "num_bvh_nodes %d for %d primitives (expected 2N-1)", s->num_bvh_nodes, np);
  if (s->ref_nodes && bad16(s->ref_nodes)) return fail(PTMI_EINVAL, "ref_nodes misaligned");
  // Shell hint (include/ptmi.h): 1 + node byte offset + child index. The
  // kernels read that node, so the offset is checked; what it claims about the
  // scene is the caller's, like a leaf code's class bits.
  if (s->shell != 0) {
    const int64_t off = ((int64_t)s->shell - 1) & ~(int64_t)1;
    if (s->shell < 0 || off % kNodeBytes != 0 || off / kNodeBytes >= s->n_inner)
      return fail(PTMI_EINVAL, "shell %d is not 1 + a node offset (multiple of %u, below %d nodes) + child index",
                  s->shell, kNodeBytes, s->n_inner);
  }
  std::memset(&d, 0, sizeof d);
  d.nodes = (const float4*)s->nodes;
  d.n_inner = s->n_inner;
  d.root_ref = (np > 0) ? s->root_ref : 0;
  for (int k = 0; k < 3; ++k) {
    d.root_min[k] = s->root_min[k];
    d.root_max[k] = s->root_max[k];
  }
  d.spheres = (const float4*)s->spheres;
  d.quads = (const float4*)s->quads;
  d.tris = (const float4*)s->tris;
  d.mats = (const float4*)s->mats;
  d.mat_base[kSphere] = 0;
  d.mat_base[kQuad] = s->num_spheres;
  d.mat_base[kTriangle] = s->num_spheres + s->num_quads;
  d.texels = s->texels;
  d.num_images = s->num_images;
  for (int k = 0; k < PTMI_MAX_IMAGES; ++k) {
    d.img_offset[k] = s->img_offset[k];
    d.img_w[k] = s->img_w[k];
    d.img_h[k] = s->img_h[k];
  }
  d.perlin_vec = (const float4*)s->perlin_vec;
  d.perlin_perm = s->perlin_perm;
  d.ref_nodes = (const float4*)s->ref_nodes;
  d.n_nodes = s->num_bvh_nodes;
  d.shell = s->max_leaf_depth <= 62 ? s->shell : 0;
  d.max_leaf_depth = s->max_leaf_depth;
  return PTMI_OK;
}

static int to_dev_frame(const ptmi_frame* f, DevFrame& d) {
  if (!f) return fail(PTMI_EINVAL, "frame is NULL");
  if (f->width <= 0 || f->height <= 0 || f->w <= 0 || f->h <= 0 || f->x0 < 0 || f->y0 < 0 ||
      f->x0 + f->w > f->width || f->y0 + f->h > f->height)
    return fail(PTMI_EINVAL, "bad window %d,%d %dx%d in %dx%d", f->x0, f->y0, f->w, f->h, f->width, f->height);
  if ((int64_t)f->width * (int64_t)f->height > (int64_t)0x7fffffff / 3)
    return fail(PTMI_ECAPACITY, "image too large");
  if (f->band_rows <= 0 || f->band_stride <= 0 || f->band_offset < 0 || f->band_offset >= f->band_stride)
    return fail(PTMI_EINVAL, "bad band partition");
  if (f->max_depth < 0 || f->max_depth > 255) return fail(PTMI_EINVAL, "max_depth must be in [0, 255]");
  std::memset(&d, 0, sizeof d);
  for (int k = 0; k < 3; ++k) {
    d.center[k] = f->cam.center[k];
    d.pixel00[k] = f->cam.pixel00[k];
    d.delta_u[k] = f->cam.delta_u[k];
    d.delta_v[k] = f->cam.delta_v[k];
    d.defocus_u[k] = f->cam.defocus_u[k];
    d.defocus_v[k] = f->cam.defocus_v[k];
    d.bg[k] = f->bg[k];
  }
  d.defocus_angle = f->cam.defocus_angle;
  d.max_depth = f->max_depth;
  d.seed = f->seed;
  d.width = f->width;
  d.height = f->height;
  d.x0 = f->x0;
  d.y0 = f->y0;
  d.w = f->w;
  d.h = f->h;
  d.band_rows = f->band_rows;
  d.band_stride = f->band_stride;
  d.band_offset = f->band_offset;
  if (f->traversal != PTMI_TRAV_STACK && f->traversal != PTMI_TRAV_STACKLESS)
    return fail(PTMI_EINVAL, "unknown traversal %d", f->traversal);
  d.traversal = f->traversal;
  int32_t n = 0;
  for (int32_t r = 0; r < f->h; ++r)
    if ((r / f->band_rows) % f->band_stride == f->band_offset) ++n;
  d.n_rows = n;
  return PTMI_OK;
}

// The stackless traversal walks the reference-layout nodes (ref_nodes).
static int check_traversal(const DevScene& sc, const DevFrame& fr) {
  if (fr.traversal == PTMI_TRAV_STACKLESS && sc.n_nodes > 0 && !sc.ref_nodes)
    return fail(PTMI_EINVAL, "the stackless traversal needs the scene's ref_nodes");
  return PTMI_OK;
}

// ---------------------------------------------------------------- shared checks
// The prologue of every call that takes a scene (pt_args.hpp).
int ptmi::to_dev(const ptmi_scene_view* scene, const ptmi_frame* frame, DevScene& sc, DevFrame& fr) {
  if (int rc = to_dev_scene(scene, sc)) return rc;
  if (int rc = to_dev_frame(frame, fr)) return rc;
  return check_traversal(sc, fr);
}

static int check_accum(const float* accum) { return accum ? PTMI_OK : fail(PTMI_EINVAL, "accum is NULL"); }
static int check_stats(const float* stats) {
  return bad16(stats) ? fail(PTMI_EINVAL, "stats NULL/misaligned") : PTMI_OK;
}

// batch: the workspace of one whole batch (the trace / resolve halves), not of one sample.
static int check_workspace(const void* ws, size_t bytes, size_t need, bool batch) {
  if (!bad16(ws) && bytes >= need) return PTMI_OK;
  return fail(PTMI_EINVAL, "workspace too small/misaligned%s (%zu < %zu)", batch ? " for one batch" : "", bytes, need);
}

static bool bad_tile_count(int32_t n_tiles, const DevFrame& fr) {
  return n_tiles < 0 || n_tiles > tile_grid(fr).ntiles;
}

// ------------------------------- one body per group of entry points (`what` names the public one)
// Each keeps one order: scene, frame, traversal, the call's own arguments as
// declared, then the no-op returns around the workspace check.
// ptmi_mk_render_ws, ptmi_wf_render, ptmi_wf_render_stats, ptmi_wf_render_tiles_stats (the call has a tile list)
enum RenderKind { kMkStaged, kWf, kWfStats, kWfTilesStats };

static int render_ws_any(const char* what, RenderKind kind, const ptmi_scene_view* scene, const ptmi_frame* frame,
                         void* ws, size_t ws_bytes, float* accum, float* stats, int32_t s_begin, int32_t s_count,
                         uint64_t* counters, void* stream, const int32_t* tile_list = nullptr, int32_t n_tiles = 0) {
  DevScene sc;
  DevFrame fr;
  if (int rc = to_dev(scene, frame, sc, fr)) return rc;
  if (int rc = check_accum(accum)) return rc;
  const bool listed = kind == kWfTilesStats;
  if (kind == kWfStats || listed)
    if (int rc = check_stats(stats)) return rc;
  if (listed && bad_tile_count(n_tiles, fr))
    return fail(PTMI_EINVAL, "n_tiles %d outside [0, %lld]", n_tiles, (long long)tile_grid(fr).ntiles);
  if (listed && n_tiles > 0 && bad4(tile_list))
    return fail(PTMI_EINVAL, "tile_list NULL/misaligned");
  if (s_begin < 0 || s_count < 0) return fail(PTMI_EINVAL, "bad sample range");
  const int32_t npix = fr.w * fr.n_rows;
  if (npix == 0) return PTMI_OK;
  const size_t need = kind == kMkStaged ? mk_workspace_bytes(npix, 1) : wf_workspace_bytes(fr, 1);
  if (int rc = check_workspace(ws, ws_bytes, need, false)) return rc;
  if (s_count == 0 || (listed && n_tiles == 0)) return PTMI_OK;
  unsigned long long* cnt = (unsigned long long*)counters;
  const hipStream_t st = (hipStream_t)stream;
  const int32_t slots = stack_needed(scene);
  return check_hip(kind == kMkStaged ? mk_render_staged(sc, fr, slots, ws, ws_bytes, accum, s_begin, s_count, cnt, st)
                                     : wf_render(sc, fr, slots, ws, ws_bytes, accum, s_begin, s_count, cnt, st, stats,
                                                 listed ? tile_list : nullptr, listed ? n_tiles : 0),
                   what);
}

// ptmi_mk_trace_ws / ptmi_mk_trace_tiles_ws (listed: the call has a tile list).
static int mk_trace_any(const char* what, bool listed, const ptmi_scene_view* scene, const ptmi_frame* frame, void* ws,
                        size_t ws_bytes, const int32_t* tile_list, int32_t n_tiles, int32_t s_begin, int32_t s_count,
                        uint64_t* counters, void* stream) {
  DevScene sc;
  DevFrame fr;
  if (int rc = to_dev(scene, frame, sc, fr)) return rc;
  if (s_begin < 0 || s_count < 1) return fail(PTMI_EINVAL, "bad sample range");
  if (listed && bad_tile_count(n_tiles, fr))
    return fail(PTMI_EINVAL, "n_tiles %d outside [0, %lld]", n_tiles, (long long)tile_grid(fr).ntiles);
  if (listed && n_tiles > 0 && bad4(tile_list))
    return fail(PTMI_EINVAL, "tile_list NULL/misaligned");
  const int32_t npix = fr.w * fr.n_rows;
  if (npix == 0) return PTMI_OK;
  if ((int64_t)s_count > mk_max_batch(fr))
    return fail(PTMI_ECAPACITY, "%d samples exceed one batch's 2^32 item ids", s_count);
  if (int rc = check_workspace(ws, ws_bytes, mk_workspace_bytes(npix, s_count), true)) return rc;
  if (listed && n_tiles == 0) return PTMI_OK;
  return check_hip(mk_trace_staged(sc, fr, stack_needed(scene), ws, tile_list, n_tiles, s_begin, s_count,
                                   (unsigned long long*)counters, (hipStream_t)stream),
                   what);
}

// ptmi_mk_resolve_ws / ptmi_mk_resolve_stats_ws (with_stats: the call has stats and an optional tile list).
static int mk_resolve_any(const char* what, bool with_stats, const ptmi_frame* frame, const void* ws, size_t ws_bytes,
                          float* accum, float* stats, const int32_t* tile_list, int32_t n_tiles, int32_t s_count,
                          void* stream) {
  DevFrame fr;
  if (int rc = to_dev_frame(frame, fr)) return rc;
  if (int rc = check_accum(accum)) return rc;
  if (with_stats)
    if (int rc = check_stats(stats)) return rc;
  if (s_count < 1) return fail(PTMI_EINVAL, "sample_count must be >= 1");
  if (tile_list && (bad4(tile_list) || bad_tile_count(n_tiles, fr)))
    return fail(PTMI_EINVAL, "tile_list misaligned or n_tiles %d outside [0, %lld]", n_tiles,
                (long long)tile_grid(fr).ntiles);
  const int32_t npix = fr.w * fr.n_rows;
  if (npix == 0) return PTMI_OK;
  if (int rc = check_workspace(ws, ws_bytes, mk_workspace_bytes(npix, s_count), true)) return rc;
  if (tile_list && n_tiles == 0) return PTMI_OK;
  const float* staging = (const float*)ws;
  const hipStream_t st = (hipStream_t)stream;
  return check_hip(with_stats ? launch_stats_resolve(fr, staging, npix, s_count, accum, stats, tile_list, n_tiles,
                                                     kProfMkResolve, st)
                              : launch_stage_resolve(fr, staging, npix, s_count, accum, kProfMkResolve, st),
                   what);
}

// ptmi_clear (buf = accum) / ptmi_stats_clear (buf = stats).
static int clear_any(bool is_stats, const ptmi_frame* frame, float* buf, void* stream) {
  DevFrame fr;
  if (int rc = to_dev_frame(frame, fr)) return rc;
  if (int rc = is_stats ? check_stats(buf) : check_accum(buf)) return rc;
  const int32_t npix = fr.w * fr.n_rows;
  if (npix == 0) return PTMI_OK;
  const dim3 grid = capped_grid(npix, kBlock);
  if (is_stats)
    hipLaunchKernelGGL(stats_clear_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, fr, (float4*)buf);
  else
    hipLaunchKernelGGL(clear_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, fr, buf);
  return check_hip(hipGetLastError(), is_stats ? "stats clear launch" : "clear launch");
}

// ptmi_tonemap (one spp for the image) / ptmi_tonemap_stats (with_stats: each pixel's own count).
static int tonemap_any(bool with_stats, const float* accum, const float* stats, uint8_t* out, int32_t width,
                       int32_t height, int32_t spp, void* stream) {
  if (!accum || !out || width <= 0 || height <= 0) return fail(PTMI_EINVAL, "bad tonemap arguments");
  if (with_stats)
    if (int rc = check_stats(stats)) return rc;
  const int64_t n = (int64_t)width * height * 3;
  if (n > 0x7fffffff) return fail(PTMI_ECAPACITY, "image too large");
  const float scale = (float)(1.0 / (double)(spp > 1 ? spp : 1));  // python float -> f32 (NEP 50)
  const dim3 grid = capped_grid(n, kBlock);
  if (with_stats)
    hipLaunchKernelGGL(tonemap_stats_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, accum, (const float4*)stats,
                       out, (int32_t)n);
  else
    hipLaunchKernelGGL(tonemap_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, accum, out, (int32_t)n, scale);
  return check_hip(hipGetLastError(), with_stats ? "tonemap_stats launch" : "tonemap launch");
}

extern "C" {

int ptmi_version(void) { return PTMI_ABI_VERSION; }

int ptmi_node_bytes(void) { return (int)kNodeBytes; }

const char* ptmi_last_error(void) { return g_err.c_str(); }

int ptmi_scene_check(const ptmi_scene_view* scene) {
  DevScene d;
  return to_dev_scene(scene, d);
}

int ptmi_mk_render(const ptmi_scene_view* scene, const ptmi_frame* frame, float* accum, int32_t sample_begin,
                   int32_t sample_count, uint64_t* counters, void* stream) {
  DevScene sc;
  DevFrame fr;
  if (int rc = to_dev(scene, frame, sc, fr)) return rc;
  if (int rc = check_accum(accum)) return rc;
  if (sample_begin < 0 || sample_count < 0) return fail(PTMI_EINVAL, "bad sample range");
  if (sample_count == 0 || fr.n_rows == 0) return PTMI_OK;
  return check_hip(mk_render(sc, fr, stack_needed(scene), accum, sample_begin, sample_count,
                             (unsigned long long*)counters, (hipStream_t)stream),
                   "mk_render launch");
}

size_t ptmi_mk_workspace_bytes(const ptmi_frame* frame, int32_t batch_samples) {
  DevFrame fr;
  if (to_dev_frame(frame, fr)) return 0;
  if (batch_samples <= 0) {
    fail(PTMI_EINVAL, "batch_samples must be > 0");
    return 0;
  }
  return mk_workspace_bytes(fr.w * fr.n_rows, batch_samples);
}

int ptmi_mk_render_ws(const ptmi_scene_view* scene, const ptmi_frame* frame, void* workspace,
                      size_t workspace_bytes, float* accum, int32_t sample_begin, int32_t sample_count,
                      uint64_t* counters, void* stream) {
  return render_ws_any("mk_render_ws", kMkStaged, scene, frame, workspace, workspace_bytes, accum, nullptr,
                       sample_begin, sample_count, counters, stream);
}

int ptmi_mk_trace_ws(const ptmi_scene_view* scene, const ptmi_frame* frame, void* workspace, size_t workspace_bytes,
                     int32_t sample_begin, int32_t sample_count, uint64_t* counters, void* stream) {
  return mk_trace_any("mk_trace_ws", false, scene, frame, workspace, workspace_bytes, nullptr, 0, sample_begin,
                      sample_count, counters, stream);
}

int64_t ptmi_mk_max_batch(const ptmi_frame* frame) {
  DevFrame fr;
  if (to_dev_frame(frame, fr)) return 0;
  return mk_max_batch(fr);
}

int ptmi_mk_resolve_ws(const ptmi_frame* frame, const void* workspace, size_t workspace_bytes, float* accum,
                       int32_t sample_count, void* stream) {
  return mk_resolve_any("mk_resolve_ws", false, frame, workspace, workspace_bytes, accum, nullptr, nullptr, 0,
                        sample_count, stream);
}

size_t ptmi_wf_workspace_bytes(const ptmi_frame* frame, int32_t batch_samples) {
  DevFrame fr;
  if (to_dev_frame(frame, fr)) return 0;
  if (batch_samples <= 0) {
    fail(PTMI_EINVAL, "batch_samples must be > 0");
    return 0;
  }
  if ((int64_t)fr.w * fr.n_rows * batch_samples > 0x7fffffff) {
    fail(PTMI_ECAPACITY, "pixels x batch_samples exceeds 2^31 work items");
    return 0;
  }
  return wf_workspace_bytes(fr, batch_samples);
}

int ptmi_wf_render(const ptmi_scene_view* scene, const ptmi_frame* frame, void* workspace, size_t workspace_bytes,
                   float* accum, int32_t sample_begin, int32_t sample_count, uint64_t* counters, void* stream) {
  return render_ws_any("wf_render", kWf, scene, frame, workspace, workspace_bytes, accum, nullptr, sample_begin,
                       sample_count, counters, stream);
}

int ptmi_wf_set_drain_at(int32_t divisor) {
  if (divisor < 0) return fail(PTMI_EINVAL, "drain divisor must be >= 0");
  return wf_set_drain_at(divisor);
}

int ptmi_clear(const ptmi_frame* frame, float* accum, void* stream) { return clear_any(false, frame, accum, stream); }

int ptmi_tonemap(const float* accum, uint8_t* out, int32_t width, int32_t height, int32_t spp, void* stream) {
  return tonemap_any(false, accum, nullptr, out, width, height, spp, stream);
}

// ------------------------------------------------------------- adaptive (ABI v8)
int ptmi_mk_tile_grid(const ptmi_frame* frame, int32_t* tile_w, int32_t* tile_h, int32_t* tiles_x, int32_t* tiles_y) {
  DevFrame fr;
  if (int rc = to_dev_frame(frame, fr)) return rc;
  if (!tile_w || !tile_h || !tiles_x || !tiles_y) return fail(PTMI_EINVAL, "tile grid output is NULL");
  const TileGrid g = tile_grid(fr);
  *tile_w = 1 << g.tw_log2;
  *tile_h = 64 >> g.tw_log2;
  *tiles_x = g.tiles_x;
  *tiles_y = g.tiles_x > 0 ? g.ntiles / g.tiles_x : 0;
  return PTMI_OK;
}

int ptmi_stats_clear(const ptmi_frame* frame, float* stats, void* stream) {
  return clear_any(true, frame, stats, stream);
}

int ptmi_mk_trace_tiles_ws(const ptmi_scene_view* scene, const ptmi_frame* frame, void* workspace,
                           size_t workspace_bytes, const int32_t* tile_list, int32_t n_tiles, int32_t sample_begin,
                           int32_t sample_count, uint64_t* counters, void* stream) {
  return mk_trace_any("mk_trace_tiles_ws", true, scene, frame, workspace, workspace_bytes, tile_list, n_tiles,
                      sample_begin, sample_count, counters, stream);
}

int ptmi_mk_resolve_stats_ws(const ptmi_frame* frame, const void* workspace, size_t workspace_bytes, float* accum,
                             float* stats, const int32_t* tile_list, int32_t n_tiles, int32_t sample_count,
                             void* stream) {
  return mk_resolve_any("mk_resolve_stats_ws", true, frame, workspace, workspace_bytes, accum, stats, tile_list,
                        n_tiles, sample_count, stream);
}

int ptmi_wf_render_stats(const ptmi_scene_view* scene, const ptmi_frame* frame, void* workspace,
                         size_t workspace_bytes, float* accum, float* stats, int32_t sample_begin,
                         int32_t sample_count, uint64_t* counters, void* stream) {
  return render_ws_any("wf_render_stats", kWfStats, scene, frame, workspace, workspace_bytes, accum, stats,
                       sample_begin, sample_count, counters, stream);
}

// ------------------------------------------------------------- include/ptmi_wf_tiles.h
int ptmi_wf_render_tiles_stats(const ptmi_scene_view* scene, const ptmi_frame* frame, void* workspace,
                               size_t workspace_bytes, float* accum, float* stats, const int32_t* tile_list,
                               int32_t n_tiles, int32_t sample_begin, int32_t sample_count, uint64_t* counters,
                               void* stream) {
  return render_ws_any("wf_render_tiles_stats", kWfTilesStats, scene, frame, workspace, workspace_bytes, accum, stats,
                       sample_begin, sample_count, counters, stream, tile_list, n_tiles);
}

int ptmi_tile_update(const ptmi_frame* frame, const float* stats, float threshold, int32_t min_spp, int32_t max_spp,
                     int32_t* tile_state, float* tile_err, int32_t* tile_list, int32_t* n_active, void* stream) {
  DevFrame fr;
  if (int rc = to_dev_frame(frame, fr)) return rc;
  if (int rc = check_stats(stats)) return rc;
  if (!(threshold >= 0.0f)) return fail(PTMI_EINVAL, "threshold must be >= 0");
  if (min_spp < 0 || max_spp < min_spp) return fail(PTMI_EINVAL, "bad spp range [%d, %d]", min_spp, max_spp);
  if (bad4(tile_state) || bad4(tile_err) || bad4(tile_list) || bad4(n_active))
    return fail(PTMI_EINVAL, "tile buffers NULL/misaligned");
  return check_hip(launch_tile_update(fr, stats, threshold, min_spp, max_spp, tile_state, tile_err, tile_list,
                                      n_active, (hipStream_t)stream),
                   "tile_update");
}

int ptmi_tonemap_stats(const float* accum, const float* stats, uint8_t* out, int32_t width, int32_t height,
                       void* stream) {
  return tonemap_any(true, accum, stats, out, width, height, 0, stream);
}

int ptmi_prof_start(int32_t max_launches) {
  if (max_launches < 0) return fail(PTMI_EINVAL, "max_launches < 0");
  if (prof_start(max_launches)) return fail(PTMI_EHIP, "hipEventCreate failed");
  return PTMI_OK;
}

int ptmi_prof_stop(double* ms_by_kernel, uint64_t* launches_by_kernel, int32_t n_kinds) {
  return ptmi_prof_stop_busy(ms_by_kernel, nullptr, launches_by_kernel, n_kinds);
}

int ptmi_prof_stop_busy(double* ms_by_kernel, double* busy_ms_by_kernel, uint64_t* launches_by_kernel,
                        int32_t n_kinds) {
  if (!ms_by_kernel || !launches_by_kernel || n_kinds < 0) return fail(PTMI_EINVAL, "bad arguments");
  int rc = prof_stop(ms_by_kernel, busy_ms_by_kernel, launches_by_kernel, n_kinds < kProfKinds ? n_kinds : kProfKinds);
  for (int32_t k = kProfKinds; k < n_kinds; ++k) {
    ms_by_kernel[k] = 0.0;
    launches_by_kernel[k] = 0;
    if (busy_ms_by_kernel) busy_ms_by_kernel[k] = 0.0;
  }
  if (rc < 0) return fail(PTMI_EHIP, "event timing failed");
  if (rc > 0) return fail(PTMI_ECAPACITY, "more launches than the profiling pool; counts truncated");
  return PTMI_OK;
}

}  // extern "C"
