// pt_tree.hip — the tree-quality ABI (include/ptmi_tree.h): how far a refitted
// BVH's boxes have grown since the tree was built, and the id remap that
// carries a history across a rebuild.
//
//   * tree_areas: one lane per ref_nodes row, its box area.
//   * tree_growth: one 1024-lane workgroup. Each lane walks its rows in
//     ascending order with an f64 sum, an f32 maximum and a count of its own;
//     an LDS tree behind __syncthreads() folds them for s = 512 .. 1; lane 0
//     writes {mean, max, n, 0}. The order is a function of num_bvh_nodes alone,
//     so the result is reproducible bit for bit. One workgroup: the trees here
//     have under 7 k nodes and the call sits beside a 45-us refit
//     (profiles/rebuild/timing.json has its time on a 2^20-sphere tree).
//   * ids_remap: one lane per id of an id image.
//
// The arithmetic is pt_tree_math.hpp's, shared with tree_check.cpp. Nothing is
// timed by ptmi_prof_*. No render kernel is involved.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_tree.h"
#include "pt_args.hpp"
#include "pt_tree_math.hpp"

namespace ptmi {

constexpr int kTreeBlock = 256;
constexpr int kGrowthLanes = PTMI_TREE_GROWTH_LANES;

__global__ __launch_bounds__(kTreeBlock) void tree_areas(const float* __restrict__ ref_nodes,
                                                         float* __restrict__ areas, int32_t n_nodes) {
  const uint32_t i = blockIdx.x * (uint32_t)kTreeBlock + threadIdx.x;
  if (i >= (uint32_t)n_nodes) return;
  areas[i] = tree_area(ref_nodes + (size_t)i * kTreeRefFloats);
}

__global__ __launch_bounds__(kGrowthLanes) void tree_growth(const float* __restrict__ ref_nodes,
                                                            const float* __restrict__ base, int32_t n_nodes,
                                                            float* __restrict__ out) {
  __shared__ double s_sum[kGrowthLanes];
  __shared__ float s_max[kGrowthLanes];
  __shared__ int32_t s_n[kGrowthLanes];
  const int k = (int)threadIdx.x;
  TreeAcc a = tree_lane(ref_nodes, base, n_nodes, k, kGrowthLanes);
  s_sum[k] = a.sum;
  s_max[k] = a.mx;
  s_n[k] = a.n;
  for (int s = kGrowthLanes / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (k < s) {
      const TreeAcc b = {s_sum[k + s], s_max[k + s], s_n[k + s]};
      tree_combine(a, b);
      s_sum[k] = a.sum;
      s_max[k] = a.mx;
      s_n[k] = a.n;
    }
  }
  if (k == 0) tree_finish(a, out);
}

__global__ __launch_bounds__(kTreeBlock) void ids_remap(const int32_t* ids_in, int32_t* ids_out, int32_t n,
                                                        TreeMaps maps) {
  const uint32_t i = blockIdx.x * (uint32_t)kTreeBlock + threadIdx.x;
  if (i >= (uint32_t)n) return;
  ids_out[i] = tree_remap_id(ids_in[i], maps);  // ids_in may be ids_out: a lane's own element
}

// The scene checks the two tree calls share.
static int tree_scene(const char* call, const ptmi_scene_view* scene) {
  if (!scene) return fail(PTMI_EINVAL, "%s: scene is NULL", call);
  if (scene->num_bvh_nodes < 0) return fail(PTMI_EINVAL, "%s: num_bvh_nodes is negative", call);
  if (scene->num_bvh_nodes > 0 && bad4(scene->ref_nodes))
    return fail(PTMI_EINVAL, "%s: ref_nodes NULL/misaligned", call);
  return PTMI_OK;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_tree_areas(const ptmi_scene_view* scene, float* areas, void* stream) {
  if (int rc = tree_scene("tree_areas", scene)) return rc;
  const int32_t n = scene->num_bvh_nodes;
  if (n == 0) return PTMI_OK;
  if (bad4(areas)) return fail(PTMI_EINVAL, "tree_areas: areas NULL/misaligned");
  hipLaunchKernelGGL(tree_areas, dim3((unsigned)(((int64_t)n + kTreeBlock - 1) / kTreeBlock)), dim3(kTreeBlock), 0,
                     (hipStream_t)stream, scene->ref_nodes, areas, n);
  return hip_result(hipGetLastError());
}

int ptmi_tree_growth(const ptmi_scene_view* scene, const float* base_areas, float* out, void* stream) {
  if (int rc = tree_scene("tree_growth", scene)) return rc;
  const int32_t n = scene->num_bvh_nodes;
  if (n > 0 && bad4(base_areas)) return fail(PTMI_EINVAL, "tree_growth: base_areas NULL/misaligned");
  if (bad4(out)) return fail(PTMI_EINVAL, "tree_growth: out NULL/misaligned");
  // with n == 0 no lane reads ref_nodes or base_areas, and lane 0 writes {1, 1, 0, 0}
  hipLaunchKernelGGL(tree_growth, dim3(1), dim3(kGrowthLanes), 0, (hipStream_t)stream, scene->ref_nodes, base_areas, n,
                     out);
  return hip_result(hipGetLastError());
}

int ptmi_ids_remap(const int32_t* ids_in, int32_t* ids_out, int32_t n, const int32_t* map_spheres,
                   const int32_t* map_tris, const int32_t* map_quads, ptmi_ids_counts counts, void* stream) {
  if (n < 0) return fail(PTMI_EINVAL, "ids_remap: n is negative");
  if (counts.spheres < 0 || counts.triangles < 0 || counts.quads < 0)
    return fail(PTMI_EINVAL, "ids_remap: a count is negative");
  if (counts.spheres > 0 && bad4(map_spheres)) return fail(PTMI_EINVAL, "ids_remap: map_spheres NULL/misaligned");
  if (counts.triangles > 0 && bad4(map_tris)) return fail(PTMI_EINVAL, "ids_remap: map_tris NULL/misaligned");
  if (counts.quads > 0 && bad4(map_quads)) return fail(PTMI_EINVAL, "ids_remap: map_quads NULL/misaligned");
  if (n == 0) return PTMI_OK;
  if (bad4(ids_in)) return fail(PTMI_EINVAL, "ids_remap: ids_in NULL/misaligned");
  if (bad4(ids_out)) return fail(PTMI_EINVAL, "ids_remap: ids_out NULL/misaligned");
  if (ids_in != ids_out && overlaps(ids_in, 4 * (uint64_t)n, ids_out, 4 * (uint64_t)n))
    return fail(PTMI_EINVAL, "ids_remap: ids_in and ids_out overlap without being equal");
  const TreeMaps maps = {map_spheres, map_tris, map_quads, counts.spheres, counts.triangles, counts.quads};
  hipLaunchKernelGGL(ids_remap, dim3((unsigned)(((int64_t)n + kTreeBlock - 1) / kTreeBlock)), dim3(kTreeBlock), 0,
                     (hipStream_t)stream, ids_in, ids_out, n, maps);
  return hip_result(hipGetLastError());
}

}  // extern "C"
