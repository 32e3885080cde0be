// pt_pose_math.hpp — the arithmetic of the pose ABI (include/ptmi_pose.h): a
// tracked primitive put where it is at shutter time t. Every point is p + t * d
// in f64, two roundings, then one cast to f32 (round to nearest): what
// ptmi/pose.py's posed objects give through the scene compiler. Each function
// writes the row floats that change, fills the builder-form record from the new
// f32 points and what the row keeps, and returns the leaf box by
// pt_update_math.hpp's rules (upd_leaves' own, pad included). Shared by
// pose_leaves (pt_pose.hip) and the CPU program pose_check.cpp.
//
// Compiled with -ffp-contract=off: one rounding per operation, as on the host.
#ifndef PT_POSE_MATH_HPP
#define PT_POSE_MATH_HPP

#include "pt_update_math.hpp"

namespace ptmi {

PTMI_UPD_HD double pose_at(double p, double d, double t) {
  const double step = t * d;
  return p + step;
}

// rec {o.xyz, d.xyz}; row {c.xyz, r}: c changes, r stays.
PTMI_UPD_HD UpdBox pose_sphere(const double* rec, double t, float* row) {
  float b[4];
  for (int k = 0; k < 3; ++k) b[k] = (float)pose_at(rec[k], rec[3 + k], t);
  b[3] = row[3];
  for (int k = 0; k < 3; ++k) row[k] = b[k];
  return upd_sphere_box(b);
}

// rec {Q.xyz, d.xyz, normal.xyz}; row {normal, D, Q, u, v, w}: D and Q change.
PTMI_UPD_HD UpdBox pose_quad(const double* rec, double t, float* row) {
  double Q[3];
  for (int k = 0; k < 3; ++k) Q[k] = pose_at(rec[k], rec[3 + k], t);
  const double xy = rec[6] * Q[0] + rec[7] * Q[1];
  const double D = xy + rec[8] * Q[2];
  float b[9];
  for (int k = 0; k < 3; ++k) b[k] = (float)Q[k];
  for (int k = 3; k < 9; ++k) b[k] = row[4 + k];  // u, v: f32 7 .. 12
  row[3] = (float)D;
  for (int k = 0; k < 3; ++k) row[4 + k] = b[k];
  return upd_quad_box(b);
}

// rec {v0, v1, v2, d}; row {v0, e1, e2, n}: v0 changes, the edges are the rest triangle's.
PTMI_UPD_HD UpdBox pose_tri(const double* rec, double t, float* row) {
  float b[9];
  for (int k = 0; k < 9; ++k) b[k] = (float)pose_at(rec[k], rec[9 + k % 3], t);
  for (int k = 0; k < 3; ++k) row[k] = b[k];
  return upd_tri_box(b);
}

}  // namespace ptmi
#endif  // PT_POSE_MATH_HPP
