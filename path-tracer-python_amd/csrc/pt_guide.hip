// pt_guide.hip — the guide trace of the guide ABI (include/ptmi_guide.h):
// first-hit guide buffers. The denoiser guided by them is
// pt_denoise.hip's filter in its GUIDED mode.
//
//   * guide_trace<STACK, TRAV>: one deterministic primary ray per pixel, one
//     lane per pixel, one wave (one block) per 8x8 pixel square, so a wave's
//     rays are coherent. Up to 4 traversals per lane (medium boundaries are
//     seen through); the LDS stack is the render kernels'. Each 32-byte guide
//     pixel is written as two 16-B stores. No cross-lane reads beyond those
//     inside traverse()'s leaf tests.
//
//   * guide_trace<STACK, TRAV, true>: the same kernel, which also writes the id
//     of the surface a pixel describes (ptmi_guide_trace_ids,
//     include/ptmi_motion.h): one more dword store per pixel. The id image is a
//     trailing kernel argument that the plain form does not have, so the plain
//     instantiations are what they were (profiles/motion/resources.md).
//
// Not timed by ptmi_prof_*.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_guide.h"
#include "../../include/ptmi_motion.h"
#include "pt_args.hpp"
#include "pt_image.hpp"
#include "pt_launch.hpp"

namespace ptmi {

constexpr int kGuideBlock = 64;  // one wave: an 8 x 8 pixel square
constexpr int kGuideSquare = 8;
constexpr int kGuideTraversals = 4;
constexpr float kGuideMissDepth = 1e10f;

// IDS: the trailing argument is the id image, int32_t* (an id form takes it, a plain one nothing).
template <int STACK, int TRAV, bool IDS = false, class... Ids>
__global__ __launch_bounds__(kGuideBlock, stress_waves(1)) void guide_trace(DevScene sc, DevFrame fr,
                                                                            float4* __restrict__ guides,
                                                                            int32_t squares_x, Ids... ids) {
  static_assert(sizeof...(Ids) == (IDS ? 1 : 0), "an id form takes its id image, a plain one nothing");
  __shared__ uint2 lds_stack[STACK * kGuideBlock];
  const int tid = threadIdx.x;
  Stack st{lds_stack + tid};
  const TileXY sq = tile_xy<kGuideSquare>(squares_x);
  const int32_t px = sq.x, py = sq.y;
  if (px >= fr.width || py >= fr.height) return;

  // get_ray (pt_device.hpp) with both jitter offsets 0 and no defocus
  const pt_v3 p00 = pt_v3f(fr.pixel00[0], fr.pixel00[1], fr.pixel00[2]);
  const pt_v3 du = pt_v3f(fr.delta_u[0], fr.delta_u[1], fr.delta_u[2]);
  const pt_v3 dv = pt_v3f(fr.delta_v[0], fr.delta_v[1], fr.delta_v[2]);
  const pt_v3 ps = pt_add(pt_add(p00, pt_scale(du, (float)px)), pt_scale(dv, (float)py));
  pt_v3 o = pt_v3f(fr.center[0], fr.center[1], fr.center[2]);
  const pt_v3 d = pt_sub(ps, o);
  const float len = sqrtf(pt_dot(d, d));

  float z = 0.0f;
  bool surface = false;
  int32_t ref = 0, g = 0;
  pt_v3 hp = o;
  for (int k = 0; k < kGuideTraversals; ++k) {
    float t = 0.0f;
    if (!traverse<STACK, kGuideBlock, TRAV>(sc, o, d, kTMin, kTMax, st, t, ref)) break;
    hp = pt_add(o, pt_scale(d, t));
    z = z + t * len;
    g = mat_index(sc, ref);
    if (!((mat_flags(sc, g) >> 8) & 1u)) {
      surface = true;
      break;
    }
    o = hp;  // a medium boundary: look through it
  }

  float4 gn = make_float4(0.0f, 0.0f, 0.0f, kGuideMissDepth), ga = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
  if (surface) {
    const pt_v3 n = hit_normal(sc, ref, hp, d);
    const Mat m = load_mat(sc, g);
    const int32_t mt = m.mat_type();
    pt_v3 a = pt_v3f(1.0f, 1.0f, 1.0f);
    if (mt == 0 || mt == 4)
      a = eval_texture(sc, ref, m, hp);
    else if (mt == 1)
      a = pt_v3f(m.m0.x, m.m0.y, m.m0.z);
    gn = make_float4(n.x, n.y, n.z, z);
    ga = make_float4(a.x, a.y, a.z, 1.0f);
  }
  const size_t p = (size_t)py * (size_t)fr.width + (size_t)px;
  guides[2 * p] = gn;
  guides[2 * p + 1] = ga;
  if constexpr (IDS) {
    // the leaf code without bit 31 and the class bits: type << 28 | prim
    int32_t* __restrict__ out = (ids, ...);
    out[p] = surface ? (leaf_type(ref) << 28 | leaf_index(ref)) : -1;
  }
}

// ids: the id image of the id form, or no argument.
template <class... Ids>
static hipError_t launch_guide_trace(const DevScene& sc, const DevFrame& fr, int32_t stack_needed, float* guides,
                                     hipStream_t stream, Ids... ids) {
  const int32_t squares_x = image_tiles_x(fr.width, kGuideSquare);
  const dim3 squares = image_tile_grid(fr.width, fr.height, kGuideSquare);  // < 2^31 / 3 pixels / 64 + edges
  return dispatch_traversal<false>(fr, stack_needed, [&](auto stack, auto trav) {
    constexpr int S = decltype(stack)::value, T = decltype(trav)::value;
    hipLaunchKernelGGL((guide_trace<S, T, sizeof...(Ids) != 0, Ids...>), squares, dim3(kGuideBlock), 0, stream, sc, fr,
                       (float4*)guides, squares_x, ids...);
    return hipGetLastError();
  });
}

// ptmi_guide_trace's checks, under the name of the entry point that makes them.
static int guide_trace_args(const char* what, const ptmi_scene_view* scene, const ptmi_frame* frame,
                            const float* guides, DevScene& sc, DevFrame& fr) {
  if (int rc = to_dev(scene, frame, sc, fr)) return rc;
  if (bad16(guides)) return fail(PTMI_EINVAL, "%s: guides NULL/misaligned", what);
  if (fr.x0 != 0 || fr.y0 != 0 || fr.w != fr.width || fr.h != fr.height)
    return fail(PTMI_EINVAL, "%s: the frame is windowed (guides are whole-frame)", what);
  if (fr.band_stride != 1) return fail(PTMI_EINVAL, "%s: the frame is banded (guides are whole-frame)", what);
  return PTMI_OK;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_guide_trace(const ptmi_scene_view* scene, const ptmi_frame* frame, float* guides, void* stream) {
  DevScene sc;
  DevFrame fr;
  if (int rc = guide_trace_args("guide_trace", scene, frame, guides, sc, fr)) return rc;
  return hip_result(launch_guide_trace(sc, fr, stack_needed(scene), guides, (hipStream_t)stream));
}

int ptmi_guide_trace_ids(const ptmi_scene_view* scene, const ptmi_frame* frame, float* guides, int32_t* ids,
                         void* stream) {
  DevScene sc;
  DevFrame fr;
  if (int rc = guide_trace_args("guide_trace_ids", scene, frame, guides, sc, fr)) return rc;
  if (bad4(ids)) return fail(PTMI_EINVAL, "guide_trace_ids: ids NULL/misaligned");
  const uint64_t n = (uint64_t)fr.width * (uint64_t)fr.height;
  if (overlaps(ids, 4 * n, guides, 32 * n)) return fail(PTMI_EINVAL, "guide_trace_ids: ids aliases guides");
  if (const char* part = scene_overlap(scene, ids, 4 * n))
    return fail(PTMI_EINVAL, "guide_trace_ids: ids aliases the scene's %s", part);
  return hip_result(launch_guide_trace(sc, fr, stack_needed(scene), guides, (hipStream_t)stream, ids));
}

}  // extern "C"
