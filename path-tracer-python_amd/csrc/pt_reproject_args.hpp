// pt_reproject_args.hpp — the argument checks ptmi_reproject (pt_reproject.hip)
// and ptmi_reproject_moved (pt_motion.hip) share, over pt_args.hpp, and the
// conversion of their cameras and parameters to the kernels' structs. Host only.
#pragma once
#include "../../include/ptmi_temporal.h"
#include "pt_args.hpp"
#include "pt_reproject_math.hpp"

namespace ptmi {

struct RpBuffer {  // a named device buffer of a call, for the overlap checks
  const char* name;
  const void* p;
  uint64_t bytes;
};

inline RpCam rp_cam(const ptmi_camera* c) {
  RpCam r;
  for (int k = 0; k < 3; ++k) {
    r.center[k] = c->center[k];
    r.pixel00[k] = c->pixel00[k];
    r.delta_u[k] = c->delta_u[k];
    r.delta_v[k] = c->delta_v[k];
  }
  return r;
}

// Everything ptmi_reproject rejects but the overlaps and the flags, with
// `what` as the message's prefix; `n` receives the pixel count.
inline int reproject_pointer_args(const char* what, const ptmi_camera* cur, const ptmi_camera* prev,
                                  const float* guides_cur, const float* guides_prev, const float* accum_prev,
                                  const float* stats_prev, int32_t width, int32_t height, const void* params,
                                  const float* accum_out, const float* stats_out, uint64_t& n) {
  if (!cur || !prev) return fail(PTMI_EINVAL, "%s: a camera is NULL", what);
  if (bad16(guides_cur)) return fail(PTMI_EINVAL, "%s: guides_cur NULL/misaligned", what);
  if (bad16(guides_prev)) return fail(PTMI_EINVAL, "%s: guides_prev NULL/misaligned", what);
  if (!accum_prev) return fail(PTMI_EINVAL, "%s: accum_prev is NULL", what);
  if (bad16(stats_prev)) return fail(PTMI_EINVAL, "%s: stats_prev NULL/misaligned", what);
  if (!params) return fail(PTMI_EINVAL, "%s: params is NULL", what);
  if (!accum_out) return fail(PTMI_EINVAL, "%s: accum_out is NULL", what);
  if (bad16(stats_out)) return fail(PTMI_EINVAL, "%s: stats_out NULL/misaligned", what);
  n = (uint64_t)image_pixels(width, height);
  if (n == 0)
    return fail(PTMI_EINVAL, "%s: bad image size (width and height >= 1, at most 2^31-1 pixels)", what);
  return PTMI_OK;
}

// An output overlapping one of the `count` inputs or the other output.
inline int reproject_overlap_args(const char* what, const RpBuffer* in, int count, const float* accum_out,
                                  const float* stats_out, uint64_t n) {
  for (int i = 0; i < count; ++i) {
    if (!in[i].p || !in[i].bytes) continue;
    if (overlaps(accum_out, 12 * n, in[i].p, in[i].bytes))
      return fail(PTMI_EINVAL, "%s: accum_out aliases %s", what, in[i].name);
    if (overlaps(stats_out, 16 * n, in[i].p, in[i].bytes))
      return fail(PTMI_EINVAL, "%s: stats_out aliases %s", what, in[i].name);
  }
  if (overlaps(accum_out, 12 * n, stats_out, 16 * n)) return fail(PTMI_EINVAL, "%s: accum_out aliases stats_out", what);
  return PTMI_OK;
}

// The value ranges of ptmi_reproject_params (its flags are the caller's).
inline int reproject_param_args(const char* what, const ptmi_reproject_params* params, RpParams& prm) {
  if (!(params->max_history >= 1.0f && params->max_history <= kRpMaxHistory))
    return fail(PTMI_EINVAL, "%s: max_history must be in [1, 2^24]", what);
  if (!(params->sigma_z >= 0.0f)) return fail(PTMI_EINVAL, "%s: sigma_z must be >= 0", what);
  if (!(params->normal_min >= -1.0f && params->normal_min <= 1.0f))
    return fail(PTMI_EINVAL, "%s: normal_min must be in [-1, 1]", what);
  if (!(params->sigma_a >= 0.0f)) return fail(PTMI_EINVAL, "%s: sigma_a must be >= 0", what);
  prm.max_history = params->max_history;
  prm.sigma_z = params->sigma_z;
  prm.normal_min = params->normal_min;
  prm.sigma_a = params->sigma_a;
  return PTMI_OK;
}

}  // namespace ptmi
