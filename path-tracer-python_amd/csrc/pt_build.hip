// pt_build.hip — the device-build ABI (include/ptmi_build.h): the binned-SAH
// builder of pt_bvh_build.cpp level by level on the device, and the packer of
// its arrays into a resident scene's tensors.
//
//   * build_sah: one 1024-lane workgroup. Every phase of pt_build_math.hpp runs
//     for lane = threadIdx.x, a __syncthreads() after each; the level loop
//     leaves when sh.nseg, one LDS word every lane reads after a barrier, is 0
//     (or the status is not), and after n levels at the latest. The phases are
//     plain loads and stores to the workspace and LDS adds: no lane reads
//     another lane's registers.
//   * build_pack: one 1024-lane workgroup, the same form: clear, copy and check, two
//     counts, gather, node rows. It leaves at once, in every lane, on a builder
//     status other than 0 (read from global memory, the same word in every
//     lane) and after the check on a rejected tree (one LDS word behind a
//     barrier).
//
// One workgroup is what PTMI_BUILD_MAX_PRIMS allows: workgroups cannot hand a
// level to each other inside one launch without a release/acquire protocol
// (DESIGN.md §17), and the host does not know the level count for separate
// launches. The arithmetic is pt_build_math.hpp's, shared with build_check.cpp.
// Nothing is timed by ptmi_prof_*. No render kernel is involved.
#include <hip/hip_runtime.h>

#include "../../include/ptmi_build.h"
#include "pt_args.hpp"
#include "pt_build_math.hpp"

namespace ptmi {

#define PTMI_BUILD_EACH(x) \
  {                        \
    x;                     \
    __syncthreads();       \
  }

__global__ __launch_bounds__(kBuildLanes) void build_sah(BuildCtx c) {
  __shared__ BuildShared sh;
  const int lane = (int)threadIdx.x;
  PTMI_BUILD_LEVELS(PTMI_BUILD_EACH, sh, c)
  if (lane == 0) build_finish(c, sh, level);
}

__global__ __launch_bounds__(kBuildLanes) void build_pack(PackCtx c) {
  __shared__ BuildShared sh;
  const int lane = (int)threadIdx.x;
  const int32_t* st = c.built.status;
  const int32_t status = st[0], n_nodes = st[1], max_leaf_depth = st[3];  // the same words in every lane
  if (status != 0 || n_nodes != c.n) {
    if (lane == 0) pack_refuse(c, PTMI_BUILD_PACK_SKIPPED);
    return;
  }
  PTMI_BUILD_EACH(pack_begin(sh, lane));
  PTMI_BUILD_EACH(pack_copy(c, sh, lane, kBuildLanes));
  for (int which = 0; which < 2; ++which) {
    PTMI_BUILD_EACH(pack_count(c, sh, which, lane));
    for (int d = 1, row = 0; d < kBuildLanes; d <<= 1, row ^= 1) PTMI_BUILD_EACH(build_scan_step(sh, lane, d, row));
    PTMI_BUILD_EACH(pack_count_finish(c, sh, which, lane, kBuildLanes));
  }
  if (sh.status != 0) {  // one LDS word, read by every lane after a barrier
    if (lane == 0) pack_refuse(c, sh.status);
    return;
  }
  PTMI_BUILD_EACH(pack_leaves(c, lane, kBuildLanes));
  pack_nodes(c, max_leaf_depth, lane, kBuildLanes);
}

static int check_arrays(const char* call, const ptmi_build_arrays* a) {
  const struct {
    const char* name;
    const void* p;
  } parts[] = {{"bbox_min", a->bbox_min}, {"bbox_max", a->bbox_max},   {"left", a->left},        {"right", a->right},
               {"parent", a->parent},     {"prim_type", a->prim_type}, {"prim_idx", a->prim_idx}};
  for (const auto& part : parts)
    if (bad4(part.p)) return fail(PTMI_EINVAL, "%s: %s NULL/misaligned", call, part.name);
  return PTMI_OK;
}

static int check_workspace(const char* call, int64_t n, const void* ws, size_t bytes) {
  if (bad16(ws)) return fail(PTMI_EINVAL, "%s: workspace NULL/misaligned", call);
  const size_t need = build_workspace_bytes((int32_t)n);
  if (bytes < need) return fail(PTMI_EINVAL, "%s: workspace of %zu bytes, %zu needed", call, bytes, need);
  return PTMI_OK;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

size_t ptmi_build_workspace_bytes(int32_t n_prims) { return build_workspace_bytes(n_prims); }

int ptmi_build_sah_device(const float* spheres, int32_t ns, const float* quads, int32_t nq, const float* tris,
                          int32_t nt, const ptmi_build_arrays* out, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream) {
  const char* call = "build_sah_device";
  if (ns < 0 || nq < 0 || nt < 0) return fail(PTMI_EINVAL, "%s: a count is negative", call);
  if (ns && bad4(spheres)) return fail(PTMI_EINVAL, "%s: spheres NULL/misaligned", call);
  if (nq && bad4(quads)) return fail(PTMI_EINVAL, "%s: quads NULL/misaligned", call);
  if (nt && bad4(tris)) return fail(PTMI_EINVAL, "%s: tris NULL/misaligned", call);
  if (bad4(status)) return fail(PTMI_EINVAL, "%s: status NULL/misaligned", call);
  const int64_t n = (int64_t)ns + nq + nt;
  if (n > PTMI_BUILD_MAX_PRIMS)
    return fail(PTMI_ECAPACITY, "%s: %lld primitives, at most %d", call, (long long)n, PTMI_BUILD_MAX_PRIMS);
  BuildCtx c = {};
  c.in = {spheres, quads, tris, ns, nq, nt};
  c.n = (int32_t)n;
  c.out.status = status;
  if (n > 0) {
    if (!out) return fail(PTMI_EINVAL, "%s: out is NULL", call);
    if (int rc = check_arrays(call, out)) return rc;
    if (int rc = check_workspace(call, n, workspace, workspace_bytes)) return rc;
    c.out = {out->bbox_min, out->bbox_max, out->left, out->right, out->parent, out->prim_type, out->prim_idx, status};
    build_carve(c.n, (char*)workspace, &c.ws);
  }
  hipLaunchKernelGGL(build_sah, dim3(1), dim3(kBuildLanes), 0, (hipStream_t)stream, c);
  return hip_result(hipGetLastError());
}

int ptmi_build_pack(const ptmi_scene_view* scene, const ptmi_build_arrays* built, const int32_t* status,
                    const ptmi_build_maps* old_row, const ptmi_build_maps* new_row, const ptmi_build_maps* perm,
                    int32_t* info, void* workspace, size_t workspace_bytes, void* stream) {
  const char* call = "build_pack";
  if (!scene) return fail(PTMI_EINVAL, "%s: scene is NULL", call);
  if (!built) return fail(PTMI_EINVAL, "%s: built is NULL", call);
  if (!old_row || !new_row || !perm) return fail(PTMI_EINVAL, "%s: a map struct is NULL", call);
  if (scene->num_spheres < 0 || scene->num_quads < 0 || scene->num_triangles < 0)
    return fail(PTMI_EINVAL, "%s: a count is negative", call);
  if (bad4(status)) return fail(PTMI_EINVAL, "%s: status NULL/misaligned", call);
  if (bad4(info)) return fail(PTMI_EINVAL, "%s: info NULL/misaligned", call);
  const int64_t n = (int64_t)scene->num_spheres + scene->num_quads + scene->num_triangles;
  if (n > PTMI_BUILD_MAX_PRIMS)
    return fail(PTMI_ECAPACITY, "%s: %lld primitives, at most %d", call, (long long)n, PTMI_BUILD_MAX_PRIMS);
  if (n == 0) return PTMI_OK;
  if (scene->num_bvh_nodes != 2 * n - 1 || scene->n_inner != n - 1)
    return fail(PTMI_EINVAL, "%s: the view's node counts are not those of %lld primitives", call, (long long)n);
  PackCtx c = {};
  c.counts[0] = scene->num_spheres, c.counts[1] = scene->num_triangles, c.counts[2] = scene->num_quads;
  c.mat_base[0] = 0, c.mat_base[2] = scene->num_spheres, c.mat_base[1] = scene->num_spheres + scene->num_quads;
  c.n_prims = (int32_t)n, c.n = 2 * (int32_t)n - 1;
  if (n > 1 && bad16(scene->nodes)) return fail(PTMI_EINVAL, "%s: nodes NULL/misaligned", call);
  if (bad4(scene->ref_nodes)) return fail(PTMI_EINVAL, "%s: ref_nodes NULL/misaligned", call);
  if (bad16(scene->mats)) return fail(PTMI_EINVAL, "%s: mats NULL/misaligned", call);
  const float* rows[3] = {scene->spheres, scene->tris, scene->quads};
  const int32_t* olds[3] = {old_row->spheres, old_row->triangles, old_row->quads};
  int32_t* news[3] = {new_row->spheres, new_row->triangles, new_row->quads};
  int32_t* perms[3] = {perm->spheres, perm->triangles, perm->quads};
  static const char* const kinds[3] = {"spheres", "triangles", "quads"};
  for (int t = 0; t < 3; ++t) {
    if (!c.counts[t]) continue;
    if (bad16(rows[t])) return fail(PTMI_EINVAL, "%s: %s rows NULL/misaligned", call, kinds[t]);
    if (bad4(olds[t])) return fail(PTMI_EINVAL, "%s: old_row %s NULL/misaligned", call, kinds[t]);
    if (bad4(news[t])) return fail(PTMI_EINVAL, "%s: new_row %s NULL/misaligned", call, kinds[t]);
    if (bad4(perms[t])) return fail(PTMI_EINVAL, "%s: perm %s NULL/misaligned", call, kinds[t]);
    c.rows[t] = const_cast<float*>(rows[t]);
    c.old_row[t] = olds[t], c.new_row[t] = news[t], c.perm[t] = perms[t];
  }
  if (int rc = check_arrays(call, built)) return rc;
  if (int rc = check_workspace(call, n, workspace, workspace_bytes)) return rc;
  c.nodes = const_cast<float*>(scene->nodes);
  c.ref_nodes = const_cast<float*>(scene->ref_nodes);
  c.mats = const_cast<float*>(scene->mats);
  c.built = {built->bbox_min, built->bbox_max, built->left,      built->right,
             built->parent,   built->prim_type, built->prim_idx, const_cast<int32_t*>(status)};
  c.info = info;
  pack_carve(c.counts, (char*)workspace, &c.ws);
  hipLaunchKernelGGL(build_pack, dim3(1), dim3(kBuildLanes), 0, (hipStream_t)stream, c);
  return hip_result(hipGetLastError());
}

}  // extern "C"
