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
// Not timed by ptmi_prof_*.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_guide.h"
#include "pt_args.hpp"
#include "pt_image.hpp"
#include "pt_launch.hpp"

namespace ptmi {

constexpr int kGuideBlock = 64;  // one wave: an 8 x 8 pixel square
constexpr int kGuideSquare = 8;
constexpr int kGuideTraversals = 4;
constexpr float kGuideMissDepth = 1e10f;

template <int STACK, int TRAV>
__global__ __launch_bounds__(kGuideBlock, stress_waves(1)) void guide_trace(DevScene sc, DevFrame fr,
                                                                            float4* __restrict__ guides,
                                                                            int32_t squares_x) {
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
}

static hipError_t launch_guide_trace(const DevScene& sc, const DevFrame& fr, int32_t stack_needed, float* guides,
                                     hipStream_t stream) {
  const int32_t squares_x = image_tiles_x(fr.width, kGuideSquare);
  const dim3 squares = image_tile_grid(fr.width, fr.height, kGuideSquare);  // < 2^31 / 3 pixels / 64 + edges
  return dispatch_traversal<false>(fr, stack_needed, [&](auto stack, auto trav) {
    constexpr int S = decltype(stack)::value, T = decltype(trav)::value;
    hipLaunchKernelGGL((guide_trace<S, T>), squares, dim3(kGuideBlock), 0, stream, sc, fr,
                       (float4*)guides, squares_x);
    return hipGetLastError();
  });
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_guide_trace(const ptmi_scene_view* scene, const ptmi_frame* frame, float* guides, void* stream) {
  DevScene sc;
  DevFrame fr;
  if (int rc = to_dev(scene, frame, sc, fr)) return rc;
  if (bad16(guides)) return fail(PTMI_EINVAL, "guide_trace: guides NULL/misaligned");
  if (fr.x0 != 0 || fr.y0 != 0 || fr.w != fr.width || fr.h != fr.height)
    return fail(PTMI_EINVAL, "guide_trace: the frame is windowed (guides are whole-frame)");
  if (fr.band_stride != 1) return fail(PTMI_EINVAL, "guide_trace: the frame is banded (guides are whole-frame)");
  return hip_result(launch_guide_trace(sc, fr, stack_needed(scene), guides, (hipStream_t)stream));
}

}  // extern "C"
