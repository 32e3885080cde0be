// pt_args.hpp — the argument checks every entry point of libptmi.so shares
// (pt_abi.hip, pt_denoise.hip, pt_guide.hip, pt_reproject.hip, pt_motion.hip,
// pt_update.hip, pt_tree.hip, pt_validate.hip, pt_material.hip, pt_pose.hip).
// Host only. The text of ptmi_last_error() and the render prologue are
// pt_abi.hip's; the rest is inline. What only the calls that edit a resident
// scene share (pt_update.hip, pt_pose.hip, pt_material.hip) is
// pt_edit_lists.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ptmi.h"

namespace ptmi {

struct DevScene;
struct DevFrame;

// Sets the calling thread's ptmi_last_error() text and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// The prologue of every call that takes a scene: scene, frame and traversal
// checks and the conversion to the kernels' structs.
int to_dev(const ptmi_scene_view* scene, const ptmi_frame* frame, DevScene& sc, DevFrame& fr);

// Traversal stack slots a scene needs.
inline int32_t stack_needed(const ptmi_scene_view* s) { return s->max_leaf_depth + 1; }

inline int hip_result(hipError_t e) {
  return e == hipSuccess ? PTMI_OK : fail(PTMI_EHIP, "%s", hipGetErrorString(e));
}

inline bool bad16(const void* p) { return !p || ((uintptr_t)p & 15u); }  // NULL or misaligned
inline bool bad8(const void* p) { return !p || ((uintptr_t)p & 7u); }
inline bool bad4(const void* p) { return !p || ((uintptr_t)p & 3u); }

// Pixels of a width x height image, 0 for a size no image kernel takes
// (a side below 1, more than 2^31-1 pixels).
inline int64_t image_pixels(int32_t width, int32_t height) {
  if (width < 1 || height < 1) return 0;
  const int64_t n = (int64_t)width * (int64_t)height;
  return n > 0x7fffffff ? 0 : n;
}

inline bool overlaps(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

// The name of the first device array of a checked scene view (include/ptmi.h's
// layouts) that [p, p + bytes) overlaps, or NULL: for a call that writes an
// image while it reads the scene.
inline const char* scene_overlap(const ptmi_scene_view* s, const void* p, uint64_t bytes) {
  uint64_t texels = 0;
  for (int32_t k = 0; k < s->num_images && k < PTMI_MAX_IMAGES; ++k) {
    const uint64_t end = (uint64_t)s->img_offset[k] + (uint64_t)s->img_w[k] * (uint64_t)s->img_h[k];
    if (end > texels) texels = end;
  }
  const uint64_t prims = (uint64_t)s->num_spheres + (uint64_t)s->num_quads + (uint64_t)s->num_triangles;
  const struct {
    const char* name;
    const void* p;
    uint64_t bytes;
  } parts[] = {{"nodes", s->nodes, (uint64_t)s->n_inner * (uint64_t)ptmi_node_bytes()},
               {"spheres", s->spheres, 16 * (uint64_t)s->num_spheres},
               {"quads", s->quads, 64 * (uint64_t)s->num_quads},
               {"tris", s->tris, 48 * (uint64_t)s->num_triangles},
               {"mats", s->mats, 80 * prims},
               {"texels", s->texels, 4 * texels},
               {"perlin_vec", s->perlin_vec, 256 * 16},
               {"perlin_perm", s->perlin_perm, 3 * 256 * 4},
               {"ref_nodes", s->ref_nodes, 48 * (uint64_t)s->num_bvh_nodes}};
  for (const auto& part : parts)
    if (part.p && part.bytes && overlaps(p, bytes, part.p, part.bytes)) return part.name;
  return nullptr;
}

}  // namespace ptmi
