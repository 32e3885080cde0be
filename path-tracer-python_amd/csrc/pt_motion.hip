// pt_motion.hip — the motion ABI's reprojection (include/ptmi_motion.h):
// a stats render's history carried across a scene update. The
// id form of the guide trace is pt_guide.hip's.
//
//   * reproject_moved: rp_reproject's geometry (pt_reproject.hip): one lane per
//     pixel of the current frame, one block per 16 x 16 pixel tile. A hit pixel
//     reads its id (one dword), checks it against the counts, and only then
//     forms the address of its primitive's current and previous row: 1, 4 or 3
//     16-B loads each (4, 16, 12 floats). Neighbouring lanes mostly see the
//     same primitive, so the row loads are served by the caches. With
//     PTMI_RPM_MATCH_IDS a tap reads one more dword. The cameras and the
//     parameters are kernel arguments. No cross-lane reads, no LDS.
//
// The arithmetic is pt_motion_math.hpp's and pt_reproject_math.hpp's, shared
// with motion_check.cpp; the kernel only decides where a value is read from.
// Not timed by ptmi_prof_*.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_motion.h"
#include "pt_image.hpp"
#include "pt_motion_math.hpp"
#include "pt_reproject_args.hpp"

namespace ptmi {

struct MvRows {  // the three row arrays of a scene, current or previous
  const float4* __restrict__ spheres;
  const float4* __restrict__ quads;
  const float4* __restrict__ tris;
};

// Row `prim` of N floats, N / 4 16-B loads. The caller has checked prim against the count.
template <int N>
__device__ __forceinline__ void load_row(const float4* __restrict__ rows, int32_t prim, float (&out)[N]) {
  static_assert(N % 4 == 0, "rows are whole float4s");
  const float4* r = rows + (size_t)prim * (N / 4);
#pragma unroll
  for (int k = 0; k < N / 4; ++k) {
    const float4 v = r[k];
    out[4 * k] = v.x;
    out[4 * k + 1] = v.y;
    out[4 * k + 2] = v.z;
    out[4 * k + 3] = v.w;
  }
}

__global__ __launch_bounds__(kImgBlock) void reproject_moved(
    RpCam cur, RpCam prev, RpParams prm, int32_t match_ids, MvCounts counts, MvRows rows_cur, MvRows rows_prev,
    const float4* __restrict__ guides_cur, const float4* __restrict__ guides_prev,
    const float* __restrict__ accum_prev, const float4* __restrict__ stats_prev, const int32_t* __restrict__ ids_cur,
    const int32_t* __restrict__ ids_prev, float* __restrict__ accum_out, float4* __restrict__ stats_out,
    int32_t width, int32_t height, int32_t tiles_x) {
  const TileXY t = tile_xy<kImgTile>(tiles_x);
  const int32_t x = t.x, y = t.y;
  if (x >= width || y >= height) return;
  auto index = [&](int32_t qx, int32_t qy) { return (size_t)qy * (size_t)width + (size_t)qx; };
  const RpOut o = mv_reproject_px(
      x, y, width, height, cur, prev, prm, match_ids != 0, counts,
      [&](int32_t qx, int32_t qy) { return load_guide(guides_cur, index(qx, qy)); },
      [&](int32_t qx, int32_t qy) { return ids_cur[index(qx, qy)]; },
      [&](RpV3 P, const MvId& m) {  // m.prim is below its type's count (mv_decode)
        if (m.type == kMvSphere) {
          float a[kMvSphereFloats], b[kMvSphereFloats];
          load_row(rows_cur.spheres, m.prim, a);
          load_row(rows_prev.spheres, m.prim, b);
          return mv_sphere_prev(P, a, b);
        }
        if (m.type == kMvQuad) {
          float a[kMvQuadFloats], b[kMvQuadFloats];
          load_row(rows_cur.quads, m.prim, a);
          load_row(rows_prev.quads, m.prim, b);
          return mv_quad_prev(P, a, b);
        }
        float a[kMvTriFloats], b[kMvTriFloats];
        load_row(rows_cur.tris, m.prim, a);
        load_row(rows_prev.tris, m.prim, b);
        return mv_tri_prev(P, a, b);
      },
      [&](int32_t qx, int32_t qy) { return load_guide(guides_prev, index(qx, qy)); },
      [&](int32_t qx, int32_t qy) {
        const float* a = accum_prev + 3 * index(qx, qy);
        return RpRgb{a[0], a[1], a[2]};
      },
      [&](int32_t qx, int32_t qy) {
        const float4 s = stats_prev[index(qx, qy)];
        return RpStats{s.x, s.y, s.z, s.w};
      },
      [&](int32_t qx, int32_t qy) { return ids_prev[index(qx, qy)]; });
  const size_t p = index(x, y);
  stats_out[p] = make_float4(o.stats.n, o.stats.mean, o.stats.m2, o.stats.pad);
  float* a = accum_out + 3 * p;
  a[0] = o.accum.r;
  a[1] = o.accum.g;
  a[2] = o.accum.b;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_reproject_moved(const ptmi_camera* cur, const ptmi_camera* prev, const float* guides_cur,
                         const float* guides_prev, const float* accum_prev, const float* stats_prev,
                         const int32_t* ids_cur, const int32_t* ids_prev, const ptmi_scene_view* scene,
                         const float* prev_spheres, const float* prev_quads, const float* prev_tris, int32_t width,
                         int32_t height, const ptmi_reproject_moved_params* params, float* accum_out,
                         float* stats_out, void* stream) {
  const char* what = "reproject_moved";
  uint64_t n = 0;
  if (int rc = reproject_pointer_args(what, cur, prev, guides_cur, guides_prev, accum_prev, stats_prev, width, height,
                                      params, accum_out, stats_out, n))
    return rc;
  if (bad4(ids_cur)) return fail(PTMI_EINVAL, "%s: ids_cur NULL/misaligned", what);
  if (bad4(ids_prev)) return fail(PTMI_EINVAL, "%s: ids_prev NULL/misaligned", what);
  if (!scene) return fail(PTMI_EINVAL, "%s: scene is NULL", what);
  const struct {
    const char *name, *prev_name;
    int32_t count;
    const float *rows, *prev_rows;
    uint64_t row_bytes;
  } kinds[3] = {{"spheres", "prev_spheres", scene->num_spheres, scene->spheres, prev_spheres, 4 * kMvSphereFloats},
                {"quads", "prev_quads", scene->num_quads, scene->quads, prev_quads, 4 * kMvQuadFloats},
                {"tris", "prev_tris", scene->num_triangles, scene->tris, prev_tris, 4 * kMvTriFloats}};
  RpBuffer in[12] = {{"guides_cur", guides_cur, 32 * n}, {"guides_prev", guides_prev, 32 * n},
                     {"accum_prev", accum_prev, 12 * n}, {"stats_prev", stats_prev, 16 * n},
                     {"ids_cur", ids_cur, 4 * n},        {"ids_prev", ids_prev, 4 * n}};
  int n_in = 6;
  for (const auto& k : kinds) {
    if (k.count < 0 || k.count > kMvMaxPrims)
      return fail(PTMI_EINVAL, "%s: the scene's count of %s is outside [0, 2^25]", what, k.name);
    if (k.count == 0) continue;
    if (bad16(k.rows)) return fail(PTMI_EINVAL, "%s: the scene's %s NULL/misaligned", what, k.name);
    if (bad16(k.prev_rows)) return fail(PTMI_EINVAL, "%s: %s NULL/misaligned", what, k.prev_name);
    in[n_in++] = RpBuffer{k.name, k.rows, k.row_bytes * (uint64_t)k.count};
    in[n_in++] = RpBuffer{k.prev_name, k.prev_rows, k.row_bytes * (uint64_t)k.count};
  }
  if (int rc = reproject_overlap_args(what, in, n_in, accum_out, stats_out, n)) return rc;
  RpParams prm;
  if (int rc = reproject_param_args(what, &params->base, prm)) return rc;
  if (params->base.flags != 0) return fail(PTMI_EINVAL, "%s: base.flags must be 0", what);
  if (params->flags & ~PTMI_RPM_MATCH_IDS) return fail(PTMI_EINVAL, "%s: unknown flag bits", what);
  const MvCounts counts = {scene->num_spheres, scene->num_quads, scene->num_triangles};
  const MvRows rows_cur = {(const float4*)scene->spheres, (const float4*)scene->quads, (const float4*)scene->tris};
  const MvRows rows_prev = {(const float4*)prev_spheres, (const float4*)prev_quads, (const float4*)prev_tris};
  hipLaunchKernelGGL(reproject_moved, image_tile_grid(width, height, kImgTile), dim3(kImgBlock), 0,
                     (hipStream_t)stream, rp_cam(cur), rp_cam(prev), prm, (int32_t)(params->flags & PTMI_RPM_MATCH_IDS),
                     counts, rows_cur, rows_prev, (const float4*)guides_cur, (const float4*)guides_prev, accum_prev,
                     (const float4*)stats_prev, ids_cur, ids_prev, accum_out, (float4*)stats_out, width, height,
                     image_tiles_x(width, kImgTile));
  return hip_result(hipGetLastError());
}

}  // extern "C"
