// pt_args.hpp — the argument checks every entry point of libptmi.so shares
// (pt_abi.hip, pt_denoise.hip, pt_guide.hip, pt_reproject.hip, pt_update.hip).
// Host only. The text of ptmi_last_error() and the render prologue are
// pt_abi.hip's; the rest is inline.
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

}  // namespace ptmi
