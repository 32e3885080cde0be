// pt_build_math.hpp — the per-lane, per-phase functions of the device builder
// and packer (include/ptmi_build.h). The kernels of pt_build.hip
// call each phase with lane = threadIdx.x and put a __syncthreads() between two
// phases; build_check.cpp calls the same functions for lane = 0 .. lanes - 1 in
// a plain loop where the kernel has its barrier. Nothing here reads another
// lane's registers, so every phase is a function of memory alone.
//
// The arithmetic is pt_bvh_build.cpp's (the recursive host builder), restated
// per level: every float expression has the host's operands in the host's
// order, leaf boxes come from pt_update_math.hpp, and every union runs over a
// segment in the order of its id array, so that a tie between -0.0 and +0.0
// falls as it does on the host (the later operand of a union wins, the first
// centroid of a min/max wins).
//
// Compiled with -ffp-contract=off and correctly rounded division.
#ifndef PT_BUILD_MATH_HPP
#define PT_BUILD_MATH_HPP

#include <stddef.h>
#include <stdint.h>

#include "../../include/ptmi_build.h"
#include "pt_material_math.hpp"
#include "pt_update_math.hpp"

#if defined(__HIPCC__)
#define PTMI_BLD_HD __host__ __device__ __forceinline__
#else
#define PTMI_BLD_HD inline
#endif

namespace ptmi {

constexpr int kBuildLanes = PTMI_BUILD_LANES;
constexpr int kBuildBuckets = 16;
constexpr int kBuildBinFloats = 7;  // a bin: box min, box max, count (as int32 bits)
constexpr int kBuildSegFloats = 12;  // a segment's reductions: box min, box max, centroid min, centroid max
constexpr int32_t kBuildFlagA = 1;  // fallback entrance (a): no finite cost, the median of c[0]
constexpr int32_t kBuildFlagB = 2;  // fallback entrance (b): a one-sided split, sort and cut at k / 2
static_assert(PTMI_BUILD_MAX_PRIMS <= 4 * kBuildLanes, "a lane scans four positions and two segments");

// Counters and the scan rows of the one workgroup (LDS on the device).
struct BuildShared {
  int32_t nseg, nseg_next, status, max_leaf_depth, fallback_a, fallback_b;
  int32_t scan[2][kBuildLanes];
};

#if defined(__HIP_DEVICE_COMPILE__)
PTMI_BLD_HD void build_add(int32_t* p, int32_t v) { atomicAdd(p, v); }
PTMI_BLD_HD void build_max(int32_t* p, int32_t v) { atomicMax(p, v); }
#else
PTMI_BLD_HD void build_add(int32_t* p, int32_t v) { *p += v; }
PTMI_BLD_HD void build_max(int32_t* p, int32_t v) { *p = *p > v ? *p : v; }
#endif

struct BuildIn {
  const float* spheres;
  const float* quads;
  const float* tris;
  int32_t ns, nq, nt;
};

struct BuildOut {
  float *bmin, *bmax;
  int32_t *left, *right, *parent, *ptype, *pidx;
  int32_t* status;  // PTMI_BUILD_STATUS_WORDS
};

// The caller's workspace, carved by build_carve. n = primitives, S = max(1, n / 2) open segments at most.
struct BuildWs {
  float* pbox;         // [n][6] leaf boxes by builder id
  float* pc;           // [n][3] centroids
  int32_t* ids[2];     // [n] the id array of a level and of the next
  int32_t* segof[2];   // [n] open segment of a position, -1 once it is a leaf
  int32_t* scan;       // [n + 1] exclusive count of left-going positions
  int32_t* sstart[2];  // [S] segments of a level and of the next
  int32_t* scount[2];
  int32_t* snode[2];
  float* sf;           // [S][12]
  int32_t* saxis;      // [S]
  float* spos;         // [S]
  int32_t* sflag;      // [S]
  int32_t* skl;        // [S] primitives going left
  int32_t* scbase;     // [S] first open child in the next level's table
  float* bins;         // [S][3][16][7]
  uint8_t* bkt;        // [n][3] bucket of a position per axis, 255 on an axis without extent
};

PTMI_BLD_HD size_t build_carve(int32_t n, char* base, BuildWs* w) {
  const size_t N = (size_t)(n > 0 ? n : 0), S = N / 2 > 0 ? N / 2 : 1;
  size_t off = 0;
  BuildWs t;
#define PTMI_BLD_TAKE(field, type, count)          \
  t.field = (type*)((uintptr_t)base + off);                   \
  off += (((count) * sizeof(type)) + 15) & ~(size_t)15;
  PTMI_BLD_TAKE(pbox, float, 6 * N)
  PTMI_BLD_TAKE(pc, float, 3 * N)
  for (int j = 0; j < 2; ++j) {
    PTMI_BLD_TAKE(ids[j], int32_t, N)
    PTMI_BLD_TAKE(segof[j], int32_t, N)
    PTMI_BLD_TAKE(sstart[j], int32_t, S)
    PTMI_BLD_TAKE(scount[j], int32_t, S)
    PTMI_BLD_TAKE(snode[j], int32_t, S)
  }
  PTMI_BLD_TAKE(scan, int32_t, N + 1)
  PTMI_BLD_TAKE(sf, float, kBuildSegFloats * S)
  PTMI_BLD_TAKE(saxis, int32_t, S)
  PTMI_BLD_TAKE(spos, float, S)
  PTMI_BLD_TAKE(sflag, int32_t, S)
  PTMI_BLD_TAKE(skl, int32_t, S)
  PTMI_BLD_TAKE(scbase, int32_t, S)
  PTMI_BLD_TAKE(bins, float, (size_t)3 * kBuildBuckets * kBuildBinFloats * S)
  PTMI_BLD_TAKE(bkt, uint8_t, 3 * N)
#undef PTMI_BLD_TAKE
  if (w) *w = t;
  return off;
}

struct BuildCtx {
  BuildIn in;
  BuildOut out;
  BuildWs ws;
  int32_t n;
};

PTMI_BLD_HD float build_inf() { return __builtin_huge_valf(); }

// The host builder's type code and index of builder id `id` (spheres, quads, triangles: codes 0, 2, 1).
PTMI_BLD_HD void build_prim(const BuildCtx& c, int32_t id, int32_t& type, int32_t& idx) {
  if (id < c.in.ns) {
    type = 0, idx = id;
  } else if (id < c.in.ns + c.in.nq) {
    type = 2, idx = id - c.in.ns;
  } else {
    type = 1, idx = id - c.in.ns - c.in.nq;
  }
}

// AABB.surface_area, pt_bvh_build.cpp's order.
PTMI_BLD_HD float build_area(const float* mn, const float* mx) {
  const float e0 = mx[0] - mn[0], e1 = mx[1] - mn[1], e2 = mx[2] - mn[2];
  float s = e0 * e1 + e1 * e2;
  s = s + e2 * e0;
  return 2.0f * s;
}

PTMI_BLD_HD void build_leaf(const BuildCtx& c, int32_t node, int32_t id) {
  for (int k = 0; k < 3; ++k) {
    c.out.bmin[3 * node + k] = c.ws.pbox[6 * id + k];
    c.out.bmax[3 * node + k] = c.ws.pbox[6 * id + 3 + k];
  }
  c.out.left[node] = -1;
  c.out.right[node] = -1;
  int32_t type, idx;
  build_prim(c, id, type, idx);
  c.out.ptype[node] = type;
  c.out.pidx[node] = idx;
}

// Phase 0: leaf boxes and centroids, the identity id array, the root segment.
PTMI_BLD_HD void build_init(const BuildCtx& c, BuildShared& sh, int lane, int lanes) {
  const int32_t n = c.n;
  if (lane == 0) {
    sh.nseg = n >= 2 ? 1 : 0;
    sh.nseg_next = 0;
    sh.status = 0;
    sh.max_leaf_depth = 0;
    sh.fallback_a = sh.fallback_b = 0;
    if (n >= 2) {
      c.ws.sstart[0][0] = 0;
      c.ws.scount[0][0] = n;
      c.ws.snode[0][0] = 0;
    }
    if (n >= 1) c.out.parent[0] = -1;
  }
  for (int32_t id = lane; id < n; id += lanes) {
    UpdBox b;
    float ct[3];
    if (id < c.in.ns) {
      const float* s = c.in.spheres + 4 * (size_t)id;
      b = upd_sphere_box(s);
      for (int k = 0; k < 3; ++k) ct[k] = s[k];
    } else if (id < c.in.ns + c.in.nq) {
      const float* q = c.in.quads + 9 * (size_t)(id - c.in.ns);
      b = upd_quad_box(q);
      for (int k = 0; k < 3; ++k) ct[k] = (q[k] + 0.5f * q[3 + k]) + 0.5f * q[6 + k];
    } else {
      const float* t = c.in.tris + 9 * (size_t)(id - c.in.ns - c.in.nq);
      b = upd_tri_box(t);
      for (int k = 0; k < 3; ++k) ct[k] = ((t[k] + t[3 + k]) + t[6 + k]) / 3.0f;
    }
    for (int k = 0; k < 3; ++k) {
      c.ws.pbox[6 * id + k] = b.mn[k];
      c.ws.pbox[6 * id + 3 + k] = b.mx[k];
      c.ws.pc[3 * id + k] = ct[k];
    }
    c.ws.ids[0][id] = id;
    c.ws.segof[0][id] = n >= 2 ? 0 : -1;
    if (n == 1) build_leaf(c, 0, id);
  }
}

// Phase A: one task per (segment, word of its 12 reductions), a walk of the segment in id order.
// Words 0 - 5: the node box (a union: the later operand wins a tie); 6 - 8 the centroid minimum and
// 9 - 11 the maximum per axis (strict comparisons: the first wins).
PTMI_BLD_HD void build_reduce(const BuildCtx& c, const BuildShared& sh, int cur, int lane, int lanes) {
  const int32_t tasks = sh.nseg * kBuildSegFloats;
  const int32_t* ids = c.ws.ids[cur];
  for (int32_t t = lane; t < tasks; t += lanes) {
    const int32_t s = t / kBuildSegFloats, w = t % kBuildSegFloats;
    const int32_t start = c.ws.sstart[cur][s], k = c.ws.scount[cur][s];
    float r;
    if (w < 3) {
      r = build_inf();
      for (int32_t q = 0; q < k; ++q) r = upd_min(r, c.ws.pbox[6 * ids[start + q] + w]);
    } else if (w < 6) {
      r = -build_inf();
      for (int32_t q = 0; q < k; ++q) r = upd_max(r, c.ws.pbox[6 * ids[start + q] + w]);
    } else if (w < 9) {
      r = c.ws.pc[3 * ids[start] + (w - 6)];
      for (int32_t q = 1; q < k; ++q) {
        const float v = c.ws.pc[3 * ids[start + q] + (w - 6)];
        if (v < r) r = v;
      }
    } else {
      r = c.ws.pc[3 * ids[start] + (w - 9)];
      for (int32_t q = 1; q < k; ++q) {
        const float v = c.ws.pc[3 * ids[start + q] + (w - 9)];
        if (v > r) r = v;
      }
    }
    c.ws.sf[kBuildSegFloats * s + w] = r;
  }
}

// Phase B: the bucket of every open position on every axis that has an extent.
PTMI_BLD_HD void build_buckets(const BuildCtx& c, int cur, int lane, int lanes) {
  for (int32_t p = lane; p < c.n; p += lanes) {
    const int32_t s = c.ws.segof[cur][p];
    if (s < 0) continue;
    const float* f = c.ws.sf + kBuildSegFloats * s;
    const int32_t id = c.ws.ids[cur][p];
    for (int a = 0; a < 3; ++a) {
      const float minc = f[6 + a], extent = f[9 + a] - minc;
      int b = 255;
      if (!(extent < 1e-10f)) {
        const float off = (c.ws.pc[3 * id + a] - minc) / extent;
        b = (int)(off * 16.0f);
        if (b > kBuildBuckets - 1) b = kBuildBuckets - 1;
        if (b < 0) b = 0;  // unreachable on finite input; keeps the byte a bucket
      }
      c.ws.bkt[3 * p + a] = (uint8_t)b;
    }
  }
}

// Phase C: one task per (segment, axis, bucket): count and box of the bucket, a walk in id order.
PTMI_BLD_HD void build_bins(const BuildCtx& c, const BuildShared& sh, int cur, int lane, int lanes) {
  const int32_t per = 3 * kBuildBuckets, tasks = sh.nseg * per;
  const int32_t* ids = c.ws.ids[cur];
  for (int32_t t = lane; t < tasks; t += lanes) {
    const int32_t s = t / per, a = (t % per) / kBuildBuckets, b = t % kBuildBuckets;
    const int32_t start = c.ws.sstart[cur][s], k = c.ws.scount[cur][s];
    float mn[3] = {build_inf(), build_inf(), build_inf()}, mx[3] = {-build_inf(), -build_inf(), -build_inf()};
    int32_t cnt = 0;
    for (int32_t q = start; q < start + k; ++q) {
      if (c.ws.bkt[3 * q + a] != b) continue;
      const float* pb = c.ws.pbox + 6 * ids[q];
      for (int j = 0; j < 3; ++j) {
        mn[j] = upd_min(mn[j], pb[j]);
        mx[j] = upd_max(mx[j], pb[3 + j]);
      }
      ++cnt;
    }
    float* bin = c.ws.bins + (size_t)t * kBuildBinFloats;
    for (int j = 0; j < 3; ++j) bin[j] = mn[j], bin[3 + j] = mx[j];
    ((int32_t*)bin)[6] = cnt;
  }
}

// Phase D: one lane per segment: the node's box, _find_best_split's 45 costs, the split position.
PTMI_BLD_HD void build_split(const BuildCtx& c, BuildShared& sh, int cur, int lane, int lanes) {
  for (int32_t s = lane; s < sh.nseg; s += lanes) {
    const float* f = c.ws.sf + kBuildSegFloats * s;
    const int32_t node = c.ws.snode[cur][s];
    for (int k = 0; k < 3; ++k) {
      c.out.bmin[3 * node + k] = f[k];
      c.out.bmax[3 * node + k] = f[3 + k];
    }
    c.out.ptype[node] = -1;
    c.out.pidx[node] = -1;
    const int NB = kBuildBuckets;
    int best_axis = 0, best_bucket = 0;
    float best_cost = build_inf();
    const float psa = build_area(f, f + 3);
    for (int a = 0; a < 3; ++a) {
      if (f[9 + a] - f[6 + a] < 1e-10f) continue;
      const float* bin = c.ws.bins + ((size_t)s * 3 + a) * NB * kBuildBinFloats;
      int32_t rc[NB - 1];
      float rb[NB - 1][6];
      float run[6] = {build_inf(), build_inf(), build_inf(), -build_inf(), -build_inf(), -build_inf()};
      int32_t rcount = 0;
      for (int i = NB - 2; i >= 0; --i) {
        const float* bi = bin + (i + 1) * kBuildBinFloats;
        rcount += ((const int32_t*)bi)[6];
        for (int j = 0; j < 3; ++j) {
          run[j] = upd_min(run[j], bi[j]);
          run[3 + j] = upd_max(run[3 + j], bi[3 + j]);
        }
        rc[i] = rcount;
        for (int j = 0; j < 6; ++j) rb[i][j] = run[j];
      }
      for (int j = 0; j < 3; ++j) run[j] = build_inf(), run[3 + j] = -build_inf();
      int32_t lcount = 0;
      for (int i = 0; i < NB - 1; ++i) {
        const float* bi = bin + i * kBuildBinFloats;
        lcount += ((const int32_t*)bi)[6];
        for (int j = 0; j < 3; ++j) {
          run[j] = upd_min(run[j], bi[j]);
          run[3 + j] = upd_max(run[3 + j], bi[3 + j]);
        }
        if (lcount == 0 || rc[i] == 0) continue;
        const float lsa = build_area(run, run + 3);
        const float rsa = build_area(rb[i], rb[i] + 3);
        float cost = 1.0f + (lsa / psa) * 1.5f * (float)lcount;
        cost = cost + (rsa / psa) * 1.5f * (float)rc[i];
        if (cost < best_cost) {
          best_cost = cost;
          best_axis = a;
          best_bucket = i;
        }
      }
    }
    int32_t flag = 0;
    float pos = 0.0f;
    if (best_cost < build_inf()) {
      const float minc = f[6 + best_axis], extent = f[9 + best_axis] - minc;
      const float step = ((float)(best_bucket + 1) * extent) / 16.0f;
      pos = minc + step;
    } else {  // the median of c[0]: build_median writes pos
      best_axis = 0;
      flag = kBuildFlagA;
      build_add(&sh.fallback_a, 1);
    }
    c.ws.saxis[s] = best_axis;
    c.ws.spos[s] = pos;
    c.ws.sflag[s] = flag;
  }
}

// The place of position p in a stable sort of its segment on `axis`, or -1 if this builder does not
// sort such a segment: equal keys throughout are the identity at any length, distinct keys a rank
// count up to PTMI_BUILD_SORT_MAX primitives.
PTMI_BLD_HD int32_t build_rank(const BuildCtx& c, int cur, int32_t s, int32_t p, int axis) {
  const int32_t start = c.ws.sstart[cur][s], k = c.ws.scount[cur][s];
  const float* f = c.ws.sf + kBuildSegFloats * s;
  if (f[6 + axis] == f[9 + axis]) return p - start;
  if (k > PTMI_BUILD_SORT_MAX) return -1;
  const int32_t* ids = c.ws.ids[cur];
  const float mine = c.ws.pc[3 * ids[p] + axis];
  int32_t r = 0;
  for (int32_t q = start; q < start + k; ++q) {
    const float v = c.ws.pc[3 * ids[q] + axis];
    r += (v < mine || (!(mine < v) && q < p)) ? 1 : 0;
  }
  return r;
}

// Phase E: entrance (a): the position that sorts to k / 2 on axis 0 gives pos.
PTMI_BLD_HD void build_median(const BuildCtx& c, BuildShared& sh, int cur, int lane, int lanes) {
  for (int32_t p = lane; p < c.n; p += lanes) {
    const int32_t s = c.ws.segof[cur][p];
    if (s < 0 || !(c.ws.sflag[s] & kBuildFlagA)) continue;
    const int32_t r = build_rank(c, cur, s, p, 0);
    if (r < 0)
      sh.status = PTMI_BUILD_NEEDS_HOST;
    else if (r == c.ws.scount[cur][s] / 2)
      c.ws.spos[s] = c.ws.pc[3 * c.ws.ids[cur][p]];
  }
}

// Phase F: a lane's four positions: which go left, counted within the lane.
PTMI_BLD_HD void build_flags(const BuildCtx& c, BuildShared& sh, int cur, int lane) {
  int32_t sum = 0;
  for (int32_t p = 4 * lane; p < 4 * lane + 4 && p < c.n; ++p) {
    const int32_t s = c.ws.segof[cur][p];
    c.ws.scan[p] = sum;
    if (s >= 0 && c.ws.pc[3 * c.ws.ids[cur][p] + c.ws.saxis[s]] < c.ws.spos[s]) ++sum;
  }
  sh.scan[0][lane] = sum;
}

// One step of the inclusive scan over the lanes' sums (d = 1, 2, 4 ... < lanes; rows alternate, row 0 first).
PTMI_BLD_HD void build_scan_step(BuildShared& sh, int lane, int d, int src) {
  sh.scan[src ^ 1][lane] = sh.scan[src][lane] + (lane >= d ? sh.scan[src][lane - d] : 0);
}
// The row that holds the inclusive sums after every step.
PTMI_BLD_HD int build_scan_row(int lanes) {
  int row = 0;
  for (int d = 1; d < lanes; d <<= 1) row ^= 1;
  return row;
}

// Phase G: the lanes' offsets added: scan[p] = left-going positions before p, scan[n] = all of them.
PTMI_BLD_HD void build_flags_finish(const BuildCtx& c, const BuildShared& sh, int lane, int lanes) {
  const int32_t* inc = sh.scan[build_scan_row(lanes)];
  const int32_t before = lane ? inc[lane - 1] : 0;
  for (int32_t p = 4 * lane; p < 4 * lane + 4 && p < c.n; ++p) c.ws.scan[p] += before;
  if (lane == 0) c.ws.scan[c.n] = inc[lanes - 1];
}

// Phase H: a lane's two segments: how many go left, entrance (b), the children's indices.
PTMI_BLD_HD void build_children(const BuildCtx& c, BuildShared& sh, int cur, int lane) {
  int32_t sum = 0;
  for (int32_t s = 2 * lane; s < 2 * lane + 2 && s < sh.nseg; ++s) {
    const int32_t start = c.ws.sstart[cur][s], k = c.ws.scount[cur][s], node = c.ws.snode[cur][s];
    int32_t kl = c.ws.scan[start + k] - c.ws.scan[start];
    if (kl == 0 || kl == k) {
      kl = k / 2;
      c.ws.sflag[s] |= kBuildFlagB;
      build_add(&sh.fallback_b, 1);
    }
    c.ws.skl[s] = kl;
    c.out.left[node] = node + 1;  // a subtree of kl primitives has 2 kl - 1 nodes
    c.out.right[node] = node + 2 * kl;
    c.out.parent[node + 1] = node;
    c.out.parent[node + 2 * kl] = node;
    c.ws.scbase[s] = sum;
    sum += (kl >= 2 ? 1 : 0) + (k - kl >= 2 ? 1 : 0);
  }
  sh.scan[0][lane] = sum;
}

// Phase I: the next level's segment table.
PTMI_BLD_HD void build_next_segments(const BuildCtx& c, BuildShared& sh, int cur, int lane, int lanes) {
  const int32_t* inc = sh.scan[build_scan_row(lanes)];
  const int32_t before = lane ? inc[lane - 1] : 0;
  const int nxt = cur ^ 1;
  for (int32_t s = 2 * lane; s < 2 * lane + 2 && s < sh.nseg; ++s) {
    const int32_t start = c.ws.sstart[cur][s], k = c.ws.scount[cur][s], node = c.ws.snode[cur][s];
    const int32_t kl = c.ws.skl[s];
    int32_t e = c.ws.scbase[s] + before;
    c.ws.scbase[s] = e;
    if (kl >= 2) {
      c.ws.sstart[nxt][e] = start;
      c.ws.scount[nxt][e] = kl;
      c.ws.snode[nxt][e] = node + 1;
      ++e;
    }
    if (k - kl >= 2) {
      c.ws.sstart[nxt][e] = start + kl;
      c.ws.scount[nxt][e] = k - kl;
      c.ws.snode[nxt][e] = node + 2 * kl;
    }
  }
  if (lane == 0) sh.nseg_next = inc[lanes - 1];
}

// Phase J: the stable partition (or the sorted cut) into the next id array; one-primitive children become leaves.
PTMI_BLD_HD void build_scatter(const BuildCtx& c, BuildShared& sh, int cur, int32_t level, int lane, int lanes) {
  const int nxt = cur ^ 1;
  for (int32_t p = lane; p < c.n; p += lanes) {
    const int32_t s = c.ws.segof[cur][p], id = c.ws.ids[cur][p];
    if (s < 0) {
      c.ws.ids[nxt][p] = id;
      c.ws.segof[nxt][p] = -1;
      continue;
    }
    const int32_t start = c.ws.sstart[cur][s], k = c.ws.scount[cur][s], node = c.ws.snode[cur][s];
    const int32_t kl = c.ws.skl[s], axis = c.ws.saxis[s];
    int32_t to;
    if (c.ws.sflag[s] & kBuildFlagB) {
      int32_t r = build_rank(c, cur, s, p, axis);
      if (r < 0) {
        sh.status = PTMI_BUILD_NEEDS_HOST;
        r = p - start;
      }
      to = start + r;
    } else {
      const int32_t before = c.ws.scan[p] - c.ws.scan[start];
      const bool goes_left = c.ws.pc[3 * id + axis] < c.ws.spos[s];
      to = goes_left ? start + before : start + kl + (p - start - before);
    }
    const bool right = to >= start + kl;
    const int32_t kc = right ? k - kl : kl, child = right ? node + 2 * kl : node + 1;
    c.ws.ids[nxt][to] = id;
    if (kc >= 2) {
      c.ws.segof[nxt][to] = c.ws.scbase[s] + ((right && kl >= 2) ? 1 : 0);
    } else {
      c.ws.segof[nxt][to] = -1;
      build_leaf(c, child, id);
      build_max(&sh.max_leaf_depth, level + 1);
    }
  }
}

// The status block, by lane 0 after the last level.
PTMI_BLD_HD void build_finish(const BuildCtx& c, const BuildShared& sh, int32_t levels) {
  int32_t* st = c.out.status;
  st[0] = sh.status;
  st[1] = sh.status ? 0 : (c.n ? 2 * c.n - 1 : 0);
  st[2] = levels;
  st[3] = sh.max_leaf_depth;
  st[4] = sh.fallback_a;
  st[5] = sh.fallback_b;
  st[6] = st[7] = 0;
}

// The whole build in the kernel's order. SYNC is __syncthreads() on the device; on the host each
// phase runs for every lane before the next starts (BUILD_EACH).
#define PTMI_BUILD_LEVELS(EACH, sh, c)                                                          \
  EACH(build_init(c, sh, lane, kBuildLanes));                                                   \
  int32_t level = 0;                                                                            \
  for (; level < c.n; ++level) {                                                                \
    if (sh.nseg == 0 || sh.status != 0) break; /* one LDS value, read by every lane after a barrier */ \
    const int cur = level & 1;                                                                  \
    EACH(build_reduce(c, sh, cur, lane, kBuildLanes));                                          \
    EACH(build_buckets(c, cur, lane, kBuildLanes));                                             \
    EACH(build_bins(c, sh, cur, lane, kBuildLanes));                                            \
    EACH(build_split(c, sh, cur, lane, kBuildLanes));                                           \
    EACH(build_median(c, sh, cur, lane, kBuildLanes));                                          \
    EACH(build_flags(c, sh, cur, lane));                                                        \
    for (int d = 1, row = 0; d < kBuildLanes; d <<= 1, row ^= 1) EACH(build_scan_step(sh, lane, d, row)); \
    EACH(build_flags_finish(c, sh, lane, kBuildLanes));                                         \
    EACH(build_children(c, sh, cur, lane));                                                     \
    for (int d = 1, row = 0; d < kBuildLanes; d <<= 1, row ^= 1) EACH(build_scan_step(sh, lane, d, row)); \
    EACH(build_next_segments(c, sh, cur, lane, kBuildLanes));                                   \
    EACH(build_scatter(c, sh, cur, level, lane, kBuildLanes));                                  \
    EACH(if (lane == 0) sh.nseg = sh.nseg_next);                                                \
  }

// ------------------------------------------------------------------ the packer
constexpr int kPackNodeFloats = kNodeFloats, kPackRefFloats = kRefFloats, kPackMatFloats = kMatFloats;
// f32 of a primitive row of include/ptmi.h by type code: sphere, triangle, quad
PTMI_BLD_HD int pack_row_floats(int t) { return t == 0 ? 4 : t == 1 ? 12 : 16; }
static_assert(2 * PTMI_BUILD_MAX_PRIMS - 1 <= 8 * kBuildLanes, "a lane counts eight nodes");
static_assert(2 * PTMI_BUILD_MAX_PRIMS - 1 < (1 << 16), "two counts share one int32");

struct PackWs {
  float* rows[3];  // the old primitive rows by type code
  float* mats;     // the old mats rows
  int32_t* scan[2];  // [n] exclusive counts, two 16-bit fields each: internal | spheres << 16, triangles | quads << 16
  int32_t* refs;   // [n] a leaf's code, an internal node's slot * 80
};

PTMI_BLD_HD size_t pack_carve(const int32_t* counts, char* base, PackWs* w) {
  const size_t N = (size_t)counts[0] + (size_t)counts[1] + (size_t)counts[2], n = N ? 2 * N - 1 : 0;
  size_t off = 0;
  PackWs t;
#define PTMI_BLD_TAKE(field, type, count)          \
  t.field = (type*)((uintptr_t)base + off);                   \
  off += (((count) * sizeof(type)) + 15) & ~(size_t)15;
  for (int k = 0; k < 3; ++k) {
    PTMI_BLD_TAKE(rows[k], float, (size_t)pack_row_floats(k) * (size_t)counts[k])
  }
  PTMI_BLD_TAKE(mats, float, (size_t)kPackMatFloats * N)
  PTMI_BLD_TAKE(scan[0], int32_t, n)
  PTMI_BLD_TAKE(scan[1], int32_t, n)
  PTMI_BLD_TAKE(refs, int32_t, n)
#undef PTMI_BLD_TAKE
  if (w) *w = t;
  return off;
}

// Both calls' workspace for n primitives: the larger of the two (the pack's with every row a quad's).
PTMI_BLD_HD size_t build_workspace_bytes(int32_t n) {
  if (n < 0 || n > PTMI_BUILD_MAX_PRIMS) return 0;
  const int32_t worst[3] = {0, 0, n};
  const size_t a = build_carve(n, nullptr, nullptr), b = pack_carve(worst, nullptr, nullptr);
  return a > b ? a : b;
}

struct PackCtx {
  float *nodes, *ref_nodes, *mats;
  float* rows[3];      // the scene's row tensors by type code
  int32_t counts[3];   // by type code
  int32_t mat_base[3];  // first mats row of a type (the blocks lie spheres, quads, triangles)
  BuildOut built;      // read only
  const int32_t* old_row[3];
  int32_t* new_row[3];
  int32_t* perm[3];
  int32_t* info;
  PackWs ws;
  int32_t n_prims, n;  // n = 2 n_prims - 1
};

// Phase 0, a phase of its own: lane 0 clears the word the check phase below sets, and no other lane
// writes it before the barrier (as in build_init).
PTMI_BLD_HD void pack_begin(BuildShared& sh, int lane) {
  if (lane == 0) sh.status = 0;
}

// Phase 1: the old rows to the workspace; the arrays checked as a preorder tree of the scene's primitives.
// Any lane that finds a fault stores PTMI_BUILD_PACK_REJECTED (the one value) in sh.status.
PTMI_BLD_HD void pack_copy(const PackCtx& c, BuildShared& sh, int lane, int lanes) {
  for (int t = 0; t < 3; ++t) {
    const int32_t words = c.counts[t] * pack_row_floats(t);
    for (int32_t i = lane; i < words; i += lanes) c.ws.rows[t][i] = c.rows[t][i];
    for (int32_t i = lane; i < c.counts[t]; i += lanes) {
      const int32_t o = c.old_row[t][i];
      if (o < 0 || o >= c.counts[t]) sh.status = PTMI_BUILD_PACK_REJECTED;
    }
  }
  for (int32_t i = lane; i < c.n_prims * kPackMatFloats; i += lanes) c.ws.mats[i] = c.mats[i];
  for (int32_t i = lane; i < c.n; i += lanes) {
    const int32_t idx = c.built.pidx[i], l = c.built.left[i], r = c.built.right[i], par = c.built.parent[i];
    bool ok = i == 0 ? par < 0 : (par >= 0 && par < i);
    if (idx >= 0) {
      const int32_t t = c.built.ptype[i];
      ok = ok && t >= 0 && t < 3 && idx < c.counts[t < 0 || t > 2 ? 0 : t] && l < 0 && r < 0;
    } else {
      ok = ok && l > i && l < c.n && r > i && r < c.n;
    }
    if (!ok) sh.status = PTMI_BUILD_PACK_REJECTED;
  }
}

PTMI_BLD_HD int32_t pack_field(const PackCtx& c, int which, int32_t i) {
  const int32_t idx = c.built.pidx[i], t = c.built.ptype[i];
  if (which == 0) return idx < 0 ? 1 : (t == 0 ? 1 << 16 : 0);
  return idx < 0 ? 0 : (t == 1 ? 1 : t == 2 ? 1 << 16 : 0);
}

// A lane's eight nodes counted (which = 0: internal nodes and sphere leaves, 1: triangle and quad leaves).
PTMI_BLD_HD void pack_count(const PackCtx& c, BuildShared& sh, int which, int lane) {
  int32_t sum = 0;
  for (int32_t i = 8 * lane; i < 8 * lane + 8 && i < c.n; ++i) {
    c.ws.scan[which][i] = sum;
    sum += pack_field(c, which, i);
  }
  sh.scan[0][lane] = sum;
}

PTMI_BLD_HD void pack_count_finish(const PackCtx& c, BuildShared& sh, int which, int lane, int lanes) {
  const int32_t* inc = sh.scan[build_scan_row(lanes)];
  const int32_t before = lane ? inc[lane - 1] : 0;
  for (int32_t i = 8 * lane; i < 8 * lane + 8 && i < c.n; ++i) c.ws.scan[which][i] += before;
  if (lane == 0) {  // every type's leaves are as many as the scene's primitives
    const int32_t all = inc[lanes - 1], lo = all & 0xffff, hi = all >> 16;
    const bool ok = which == 0 ? (lo == c.n_prims - 1 && hi == c.counts[0]) : (lo == c.counts[1] && hi == c.counts[2]);
    if (!ok) sh.status = PTMI_BUILD_PACK_REJECTED;
  }
}

// Phase 3: every leaf's rows gathered into leaf order, its code, the two maps; every node's ref.
PTMI_BLD_HD void pack_leaves(const PackCtx& c, int lane, int lanes) {
  for (int32_t i = lane; i < c.n; i += lanes) {
    const int32_t idx = c.built.pidx[i];
    if (idx < 0) {
      c.ws.refs[i] = (c.ws.scan[0][i] & 0xffff) * (kPackNodeFloats * 4);
      continue;
    }
    const int32_t t = c.built.ptype[i];
    const int32_t now = t == 0 ? c.ws.scan[0][i] >> 16 : t == 1 ? c.ws.scan[1][i] & 0xffff : c.ws.scan[1][i] >> 16;
    const int32_t old = c.old_row[t][idx];
    const int w = pack_row_floats(t);
    for (int k = 0; k < w; ++k) c.rows[t][(size_t)now * w + k] = c.ws.rows[t][(size_t)old * w + k];
    const float* m = c.ws.mats + (size_t)(c.mat_base[t] + old) * kPackMatFloats;
    float* md = c.mats + (size_t)(c.mat_base[t] + now) * kPackMatFloats;
    for (int k = 0; k < kPackMatFloats; ++k) md[k] = m[k];
    const uint32_t flags = ((const uint32_t*)m)[kPackMatFloats - 1];
    c.ws.refs[i] = (int32_t)(0x80000000u | ((uint32_t)t << 28) | (mat_class(flags) << 25) | (uint32_t)now);
    c.new_row[t][old] = now;
    c.perm[t][now] = idx;
  }
}

// Phase 4: the ref_nodes row of every node, the nodes row of every internal node, the info block.
PTMI_BLD_HD void pack_nodes(const PackCtx& c, int32_t max_leaf_depth, int lane, int lanes) {
  const BuildOut& b = c.built;
  for (int32_t i = lane; i < c.n; i += lanes) {
    const int32_t l = b.left[i], r = b.right[i], par = b.parent[i], idx = b.pidx[i];
    float* rn = c.ref_nodes + (size_t)i * kPackRefFloats;
    int32_t* rw = (int32_t*)rn;
    for (int k = 0; k < 3; ++k) rn[k] = b.bmin[3 * i + k], rn[4 + k] = b.bmax[3 * i + k];
    rw[3] = l;
    rw[7] = r;
    rw[8] = par;
    rw[9] = idx >= 0 ? c.ws.refs[i] : 0;
    rw[10] = par >= 0 ? (b.left[par] != i ? 1 : 0) : 0;
    rw[11] = 0;
    if (idx >= 0) continue;
    float* nd = c.nodes + (size_t)(c.ws.scan[0][i] & 0xffff) * kPackNodeFloats;
    UpdBox bl, br;
    for (int k = 0; k < 3; ++k) {
      bl.mn[k] = b.bmin[3 * l + k], bl.mx[k] = b.bmax[3 * l + k];
      br.mn[k] = b.bmin[3 * r + k], br.mx[k] = b.bmax[3 * r + k];
      nd[2 * k] = bl.mn[k], nd[2 * k + 1] = br.mn[k];
      nd[6 + 2 * k] = bl.mx[k], nd[6 + 2 * k + 1] = br.mx[k];
    }
    ((int32_t*)nd)[12] = c.ws.refs[l];
    ((int32_t*)nd)[13] = c.ws.refs[r];
    nd[14] = upd_centre(bl, 2), nd[15] = upd_centre(br, 2);
    nd[16] = upd_centre(bl, 0), nd[17] = upd_centre(br, 0);
    nd[18] = upd_centre(bl, 1), nd[19] = upd_centre(br, 1);
  }
  if (lane == 0) {
    c.info[0] = c.ws.refs[0];
    c.info[1] = max_leaf_depth;
    c.info[2] = c.n_prims - 1;
    c.info[3] = c.n;
    for (int k = 0; k < 3; ++k) ((float*)c.info)[4 + k] = b.bmin[k], ((float*)c.info)[7 + k] = b.bmax[k];
    c.info[10] = c.info[11] = 0;
  }
}

// The info block of a pack that wrote nothing else.
PTMI_BLD_HD void pack_refuse(const PackCtx& c, int32_t why) {
  for (int k = 0; k < PTMI_BUILD_INFO_WORDS; ++k) c.info[k] = k == 10 ? why : 0;
}

}  // namespace ptmi
#endif  // PT_BUILD_MATH_HPP
