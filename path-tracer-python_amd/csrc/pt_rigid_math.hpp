// pt_rigid_math.hpp — the arithmetic of the rigid-body pose ABI
// (include/ptmi_rigid.h): a primitive of a body put where the body's transform
// at one time takes it. A body is 15 f64 {R row-major, c, c'}; a point goes to
// R (p - c) + c', a vector to R v, every product rounded, then the sums of a row
// left to right, then one cast to f32 (round to nearest): what ptmi/rigid.py's
// posed objects give through the scene compiler. There is no sqrt, no division
// and no transcendental here: R comes from the host. Each function writes the
// row floats, fills the builder-form record from the new f32 values and returns
// the leaf box by pt_update_math.hpp's rules (upd_leaves' own, pad included).
// Shared by rigid_leaves (pt_rigid.hip) and the CPU program rigid_check.cpp.
//
// Compiled with -ffp-contract=off: one rounding per operation, as on the host.
#ifndef PT_RIGID_MATH_HPP
#define PT_RIGID_MATH_HPP

#include "pt_update_math.hpp"

namespace ptmi {

constexpr int kRigidBodyDoubles = 15;  // ptmi_rigid_body: R[9], pivot[3], pivot_t[3]

// out = R v
PTMI_UPD_HD void rigid_vec(const double* b, const double* v, double* out) {
  for (int k = 0; k < 3; ++k) {
    const double xy = b[3 * k] * v[0] + b[3 * k + 1] * v[1];
    out[k] = xy + b[3 * k + 2] * v[2];
  }
}

// out = R (p - c) + c'
PTMI_UPD_HD void rigid_point(const double* b, const double* p, double* out) {
  double q[3], r[3];
  for (int k = 0; k < 3; ++k) q[k] = p[k] - b[9 + k];
  rigid_vec(b, q, r);
  for (int k = 0; k < 3; ++k) out[k] = r[k] + b[12 + k];
}

// rec {c}; row {c.xyz, r}: c changes, r stays.
PTMI_UPD_HD UpdBox rigid_sphere(const double* rec, const double* body, float* row) {
  double c[3];
  rigid_point(body, rec, c);
  float b[4];
  for (int k = 0; k < 3; ++k) b[k] = (float)c[k];
  b[3] = row[3];
  for (int k = 0; k < 3; ++k) row[k] = b[k];
  return upd_sphere_box(b);
}

// rec {Q, u, v, normal, w}; row {normal, D, Q, u, v, w}: all of it.
PTMI_UPD_HD UpdBox rigid_quad(const double* rec, const double* body, float* row) {
  double Q[3], u[3], v[3], n[3], w[3];
  rigid_point(body, rec, Q);
  rigid_vec(body, rec + 3, u);
  rigid_vec(body, rec + 6, v);
  rigid_vec(body, rec + 9, n);
  rigid_vec(body, rec + 12, w);
  const double xy = n[0] * Q[0] + n[1] * Q[1];
  const double D = xy + n[2] * Q[2];
  float b[9];
  for (int k = 0; k < 3; ++k) {
    b[k] = (float)Q[k];
    b[3 + k] = (float)u[k];
    b[6 + k] = (float)v[k];
    row[k] = (float)n[k];
    row[13 + k] = (float)w[k];
  }
  row[3] = (float)D;
  for (int k = 0; k < 9; ++k) row[4 + k] = b[k];
  return upd_quad_box(b);
}

// rec {v0, v1, v2, e1, e2, n}; row {v0, e1, e2, n}: all of it.
PTMI_UPD_HD UpdBox rigid_tri(const double* rec, const double* body, float* row) {
  float b[9];
  for (int j = 0; j < 3; ++j) {
    double p[3], e[3];
    rigid_point(body, rec + 3 * j, p);
    rigid_vec(body, rec + 9 + 3 * j, e);
    for (int k = 0; k < 3; ++k) {
      b[3 * j + k] = (float)p[k];
      row[3 + 3 * j + k] = (float)e[k];
    }
  }
  for (int k = 0; k < 3; ++k) row[k] = b[k];
  return upd_tri_box(b);
}

}  // namespace ptmi
#endif  // PT_RIGID_MATH_HPP
