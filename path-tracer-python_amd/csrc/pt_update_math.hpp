// pt_update_math.hpp — the arithmetic of the scene-update ABI
// (include/ptmi_update.h): the leaf box of a primitive from its builder-form
// record, the union of two boxes and the centre of a box. The leaf-box rules are
// pt_bvh_build.cpp's own (add_sphere, add_quad, add_triangle, pad_to_minimums,
// there lines 210-255 and 61-71), restated once here for the device and for the
// CPU program update_check.cpp; inputs are finite by contract, so the builder's
// NaN-propagating np.minimum / np.maximum reduce to the comparisons below.
//
// Compiled with -ffp-contract=off: one rounding per operation, as on the host.
#ifndef PT_UPDATE_MATH_HPP
#define PT_UPDATE_MATH_HPP

#if defined(__HIPCC__)
#define PTMI_UPD_HD __host__ __device__ __forceinline__
#else
#define PTMI_UPD_HD inline
#endif

namespace ptmi {

struct UpdBox {
  float mn[3], mx[3];
};

PTMI_UPD_HD float upd_min(float a, float b) { return (a < b) ? a : b; }
PTMI_UPD_HD float upd_max(float a, float b) { return (a > b) ? a : b; }

// pad_to_minimums: an extent below 0.0001f becomes 0.0001f about the middle.
PTMI_UPD_HD void upd_pad(UpdBox& b) {
  const float delta = 0.0001f;
  const float half = 5e-05f;
  for (int k = 0; k < 3; ++k) {
    if (b.mx[k] - b.mn[k] < delta) {
      const float mid = (b.mn[k] + b.mx[k]) / 2.0f;
      b.mn[k] = mid - half;
      b.mx[k] = mid + half;
    }
  }
}

// s: {c.xyz, r}
PTMI_UPD_HD UpdBox upd_sphere_box(const float* s) {
  UpdBox b;
  for (int k = 0; k < 3; ++k) {
    b.mn[k] = s[k] - s[3];
    b.mx[k] = s[k] + s[3];
  }
  return b;
}

// q: {Q, u, v}; the corners Q, Q + u, Q + v, (Q + u) + v
PTMI_UPD_HD UpdBox upd_quad_box(const float* q) {
  UpdBox b;
  for (int k = 0; k < 3; ++k) {
    const float Q = q[k], u = q[3 + k], v = q[6 + k];
    const float c1 = Q + u, c2 = Q + v, c3 = (Q + u) + v;
    b.mn[k] = upd_min(upd_min(upd_min(Q, c1), c2), c3);
    b.mx[k] = upd_max(upd_max(upd_max(Q, c1), c2), c3);
  }
  upd_pad(b);
  return b;
}

// t: {v0, v1, v2}
PTMI_UPD_HD UpdBox upd_tri_box(const float* t) {
  UpdBox b;
  for (int k = 0; k < 3; ++k) {
    const float a = t[k], v1 = t[3 + k], v2 = t[6 + k];
    b.mn[k] = upd_min(upd_min(a, v1), v2);
    b.mx[k] = upd_max(upd_max(a, v1), v2);
  }
  upd_pad(b);
  return b;
}

// The box of an internal node: l is its left child's box, r its right child's.
PTMI_UPD_HD UpdBox upd_union(const UpdBox& l, const UpdBox& r) {
  UpdBox b;
  for (int k = 0; k < 3; ++k) {
    b.mn[k] = upd_min(l.mn[k], r.mn[k]);
    b.mx[k] = upd_max(l.mx[k], r.mx[k]);
  }
  return b;
}

// Component k of a box's centre, as pack_device stores it in a node row.
PTMI_UPD_HD float upd_centre(const UpdBox& b, int k) { return (b.mn[k] + b.mx[k]) * 0.5f; }

}  // namespace ptmi
#endif  // PT_UPDATE_MATH_HPP
