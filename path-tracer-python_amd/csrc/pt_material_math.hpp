// pt_material_math.hpp — the integer rules of the material-edit ABI
// (include/ptmi_material.h): the material class of a flags word, the test that
// a leaf code names a primitive, the patch of a code's class bits and the
// bound on a flags word's image index. Stated once here for the kernel of
// pt_material.hip and for the CPU program material_check.cpp.
#ifndef PT_MATERIAL_MATH_HPP
#define PT_MATERIAL_MATH_HPP

#include <stdint.h>

#include "../../include/ptmi.h"

#if defined(__HIPCC__)
#define PTMI_MAT_HD __host__ __device__ __forceinline__
#else
#define PTMI_MAT_HD inline
#endif

namespace ptmi {

constexpr int kMatFloats = 20;      // a mats row (include/ptmi.h); f32 19 is the flags word
constexpr int kMatRefFloats = 12;   // a ref_nodes row
constexpr int kMatNodeFloats = 20;  // a nodes row; f32 12 and 13 are the child refs
constexpr uint32_t kMatIndexMask = 0x1ffffffu;  // a leaf code's primitive index, bits 0 - 24
constexpr uint32_t kMatClassMask = 7u << 25;    // its material class, bits 25 - 27

// PTMI_CLASS_* of flags = mat_type | tex_type << 4 | is_medium << 8 | (image + 1) << 16.
PTMI_MAT_HD uint32_t mat_class(uint32_t flags) {
  const uint32_t mt = flags & 0xfu, tt = (flags >> 4) & 0xfu;
  if ((flags >> 8) & 1u) return PTMI_CLASS_MEDIUM;
  if (tt == 3u && (mt == 0u || mt == 4u)) return PTMI_CLASS_NOISE;
  return mt == 0u ? PTMI_CLASS_LAMBERTIAN : mt == 2u ? PTMI_CLASS_DIELECTRIC : mt == 3u ? PTMI_CLASS_EMISSIVE
                                                                                        : PTMI_CLASS_GLOSSY;
}

// Is `code` the leaf code (0x80000000 | type << 28 | class << 25 | index) of primitive `prim` of `type`?
PTMI_MAT_HD bool mat_code_names(uint32_t code, int32_t type, int32_t prim) {
  return (code >> 28) == (8u | (uint32_t)type) && (code & kMatIndexMask) == (uint32_t)prim;
}

// `code` with its class bits replaced by `cls`; nothing else changes.
PTMI_MAT_HD uint32_t mat_patch_code(uint32_t code, uint32_t cls) { return (code & ~kMatClassMask) | ((cls & 7u) << 25); }

// Does the flags word name an image the scene has? (image index + 1 in bits 16 - 31; 0: no image)
PTMI_MAT_HD bool mat_image_ok(uint32_t flags, int32_t num_images) {
  return (int32_t)(flags >> 16) <= (num_images < 0 ? 0 : num_images);
}

}  // namespace ptmi

#endif  // PT_MATERIAL_MATH_HPP
