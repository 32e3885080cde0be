// pt_scene_rows.hpp — the layout of a resident scene's rows (include/ptmi.h)
// that the calls editing a scene in place share: the f32 counts of a ref_nodes,
// a nodes and a mats row, and the fields of a leaf code. Stated once here for
// the kernels of pt_update.hip, pt_pose.hip, pt_material.hip and pt_build.hip
// and for the CPU programs material_check.cpp and build_check.cpp.
#ifndef PT_SCENE_ROWS_HPP
#define PT_SCENE_ROWS_HPP

#include <stdint.h>

#if defined(__HIPCC__)
#define PTMI_ROWS_HD __host__ __device__ __forceinline__
#else
#define PTMI_ROWS_HD inline
#endif

namespace ptmi {

constexpr int kRefFloats = 12;   // a ref_nodes row; f32 9 is a leaf's code
constexpr int kNodeFloats = 20;  // a nodes row; f32 12 and 13 are the child refs
constexpr int kMatFloats = 20;   // a mats row; f32 19 is the flags word
constexpr int kRefCode = 9;

// A leaf code: 0x80000000 | type << 28 | class << 25 | index.
constexpr uint32_t kLeafIndexMask = 0x1ffffffu;  // the primitive index, bits 0 - 24
constexpr uint32_t kLeafClassMask = 7u << 25;    // the material class, bits 25 - 27

// Is `code` the leaf code of primitive `prim` of `type`?
PTMI_ROWS_HD bool leaf_code_names(uint32_t code, int32_t type, int32_t prim) {
  return (code >> 28) == (8u | (uint32_t)type) && (code & kLeafIndexMask) == (uint32_t)prim;
}

// `code` with its class bits replaced by `cls`; nothing else changes.
PTMI_ROWS_HD uint32_t leaf_patch_class(uint32_t code, uint32_t cls) {
  return (code & ~kLeafClassMask) | ((cls & 7u) << 25);
}

}  // namespace ptmi

#endif  // PT_SCENE_ROWS_HPP
