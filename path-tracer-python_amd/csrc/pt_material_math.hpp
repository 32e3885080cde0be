// pt_material_math.hpp — the integer rules of the material-edit ABI
// (include/ptmi_material.h) that are the material's own: the material class of
// a flags word and the bound on its image index. The leaf code they go into is
// pt_scene_rows.hpp's. Stated once here for the kernel of pt_material.hip and
// for the CPU program material_check.cpp.
#ifndef PT_MATERIAL_MATH_HPP
#define PT_MATERIAL_MATH_HPP

#include <stdint.h>

#include "../../include/ptmi.h"
#include "pt_scene_rows.hpp"

#if defined(__HIPCC__)
#define PTMI_MAT_HD __host__ __device__ __forceinline__
#else
#define PTMI_MAT_HD inline
#endif

namespace ptmi {

// PTMI_CLASS_* of flags = mat_type | tex_type << 4 | is_medium << 8 | (image + 1) << 16.
PTMI_MAT_HD uint32_t mat_class(uint32_t flags) {
  const uint32_t mt = flags & 0xfu, tt = (flags >> 4) & 0xfu;
  if ((flags >> 8) & 1u) return PTMI_CLASS_MEDIUM;
  if (tt == 3u && (mt == 0u || mt == 4u)) return PTMI_CLASS_NOISE;
  return mt == 0u ? PTMI_CLASS_LAMBERTIAN : mt == 2u ? PTMI_CLASS_DIELECTRIC : mt == 3u ? PTMI_CLASS_EMISSIVE
                                                                                        : PTMI_CLASS_GLOSSY;
}

// Does the flags word name an image the scene has? (image index + 1 in bits 16 - 31; 0: no image)
PTMI_MAT_HD bool mat_image_ok(uint32_t flags, int32_t num_images) {
  return (int32_t)(flags >> 16) <= (num_images < 0 ? 0 : num_images);
}

}  // namespace ptmi

#endif  // PT_MATERIAL_MATH_HPP
