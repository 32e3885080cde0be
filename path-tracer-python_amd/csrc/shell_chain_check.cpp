// shell_chain_check.cpp — CPU run of the shell chain's expanded segment begin
// (pt_shell_chain.hpp, the functions the megakernel's SHELL kernels call)
// against the ordinary stack walk, on a device-layout scene: a stand-alone
// program, no HIP runtime call, no GPU. `make shell_chain_check` builds it
// (hipcc -x hip --cuda-host-only, so that it shares the primitive tests of
// pt_device.hpp); tests/test_shell_chain.py runs it.
//
//   shell_chain_check SHELL N_INNER ROOT_REF MAX_LEAF_DEPTH STACK nodes.f32 spheres.f32 quads.f32 tris.f32 rays.f32 out.u32
//
// rays.f32: 7 floats per ray (o, d, tmin). out.u32: 8 words per ray: the
// ordinary walk's leaf code (0 = miss), t bits and peak stack occupancy, the
// same three of the expanded walk with its finish, whether the ray took the
// expanded begin, and whether the finish tested the skipped shell. The first
// line of stdout is the chain: m, full, side, the plan for STACK slots (m,
// skip), the slot bound, then the m node offsets. Exit 0 iff the files were
// read and written and no walk overflowed kCap slots. A twelfth argument
// `table` builds the wave's table (shell_table_entry) in an array of 128
// dwords first, as the megakernel does in two VGPRs, runs the expanded begin
// and the finish from that array alone, and prints the table's kTabSize dwords
// (hex) as a second line. Without it every table entry is computed from the
// node array where it is read.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pt_check_io.hpp"
#include "pt_device.hpp"
#include "pt_shell_chain.hpp"

using namespace ptmi;

namespace {

constexpr int kCap = 256;  // slots of the program's own stack: reported, never assumed

struct Scene {
  std::vector<float> nodes, spheres, quads, tris;
  int32_t shell, n_inner, root_ref, max_leaf_depth;
};

struct Load {
  const std::vector<float>* nodes;
  uint32_t operator()(uint32_t off, uint32_t i) const { return pt_chain_u((*nodes)[off / 4u + i]); }
};

// float a of the sphere a leaf code names, 0 unless it is a sphere leaf of the array (ChainSphereLoad, pt_megakernel.hip)
struct SphereLoad {
  const std::vector<float>* spheres;
  uint32_t operator()(int32_t ref, int a) const {
    const size_t ix = (size_t)(ref & 0x01ffffff);
    if (!(ref < 0 && ((ref >> 28) & 3) == kSphere) || 4 * ix + 4 > spheres->size()) return 0u;
    return pt_chain_u((*spheres)[4 * ix + (size_t)a]);
  }
};

// the table in an array, as the megakernel keeps it in two VGPRs
struct TableLoad {
  const uint32_t* t;
  uint32_t operator()(int i) const { return t[i]; }
};

struct Entry {
  uint32_t ref;
  float E;
};

struct Walk {
  pt_v3 o, d, inv;
  float tmin, closest;
  int32_t best;
  std::vector<Entry> st;
  int peak;
  bool overflow;
  void push(uint32_t ref, float E) {
    if ((int)st.size() >= kCap) {
      overflow = true;
      return;
    }
    st.push_back(Entry{ref, E});
    if ((int)st.size() > peak) peak = (int)st.size();
  }
};

float4 f4(const std::vector<float>& v, size_t i) { return make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]); }

// trav_begin's ray set-up (pt_device.hpp)
void ray(Walk& w, pt_v3 o, pt_v3 d, float tmin) {
  w.o = o;
  w.d = d;
  w.inv = pt_v3f(fabsf(d.x) > 1e-8f ? 1.0f / d.x : 1e8f, fabsf(d.y) > 1e-8f ? 1.0f / d.y : 1e8f,
                 fabsf(d.z) > 1e-8f ? 1.0f / d.z : 1e8f);
  w.tmin = tmin;
  w.closest = kTMax;
  w.best = 0;
  w.st.clear();
  w.peak = 0;
  w.overflow = false;
}

void slab6(const Walk& w, const float* b, int c, float& E, float& X) {  // slab() on child c of a node
  const float t0x = (b[0 + c] - w.o.x) * w.inv.x, t1x = (b[6 + c] - w.o.x) * w.inv.x;
  const float t0y = (b[2 + c] - w.o.y) * w.inv.y, t1y = (b[8 + c] - w.o.y) * w.inv.y;
  const float t0z = (b[4 + c] - w.o.z) * w.inv.z, t1z = (b[10 + c] - w.o.z) * w.inv.z;
  E = pt_maxf(pt_maxf(pt_minf(t0x, t1x), pt_minf(t0y, t1y)), pt_maxf(pt_minf(t0z, t1z), w.tmin));
  X = pt_minf(pt_minf(pt_maxf(t0x, t1x), pt_maxf(t0y, t1y)), pt_maxf(t0z, t1z));
}

// trav_step until the stack is empty: one pop per pass, culled unless E <= closest
void run(const Scene& sc, Walk& w) {
  while (!w.st.empty()) {
    const Entry e = w.st.back();
    w.st.pop_back();
    if (!(e.E <= w.closest)) continue;
    const int32_t ref = (int32_t)e.ref;
    if (ref < 0) {
      const int32_t ty = (ref >> 28) & 3, ix = ref & 0x01ffffff;
      float t, tc = w.closest;
      if (ty == kSphere) {
        if (hit_sphere_t<true>(f4(sc.spheres, 4 * (size_t)ix), w.o, w.d, w.tmin, w.closest, t)) tc = t;
      } else if (ty == kQuad) {
        const size_t q = 16 * (size_t)ix;
        if (hit_quad_v<true>(f4(sc.quads, q), f4(sc.quads, q + 4), f4(sc.quads, q + 8), f4(sc.quads, q + 12), w.o, w.d,
                             w.tmin, w.closest, t))
          tc = t;
      } else {
        const size_t q = 12 * (size_t)ix;
        if (hit_tri_v<true>(f4(sc.tris, q), f4(sc.tris, q + 4), f4(sc.tris, q + 8), w.o, w.d, w.tmin, w.closest, t)) tc = t;
      }
      if (tc < w.closest) {
        w.closest = tc;
        w.best = ref;
      }
      continue;
    }
    const float* b = &sc.nodes[(size_t)ref / 4];
    float E0, X0, E1, X1;
    slab6(w, b, 0, E0, X0);
    slab6(w, b, 1, E1, X1);
    const float cx0 = (b[0] + b[6]) * 0.5f, cx1 = (b[1] + b[7]) * 0.5f;
    const float cy0 = (b[2] + b[8]) * 0.5f, cy1 = (b[3] + b[9]) * 0.5f;
    const float d0 = ((cx0 - w.o.x) * w.d.x + (cy0 - w.o.y) * w.d.y) + (b[14] - w.o.z) * w.d.z;
    const float d1 = ((cx1 - w.o.x) * w.d.x + (cy1 - w.o.y) * w.d.y) + (b[15] - w.o.z) * w.d.z;
    const bool ln = d0 < d1, h0 = X0 >= E0, h1 = X1 >= E1;
    const uint32_t r0 = pt_chain_u(b[12]), r1 = pt_chain_u(b[13]);
    if (ln) {  // far first, then near
      if (h1) w.push(r1, E1);
      if (h0) w.push(r0, E0);
    } else {
      if (h0) w.push(r0, E0);
      if (h1) w.push(r1, E1);
    }
  }
}

void begin_root(const Scene& sc, Walk& w) {  // trav_begin: the root's box is its parent-less union, the chain's box
  if (sc.n_inner == 0 && sc.root_ref >= 0) return;
  if (sc.root_ref < 0) {
    w.push((uint32_t)sc.root_ref, w.tmin);
    return;
  }
  // the root's own box: the union of its children's, which trav_begin takes from the scene view
  const float* b = &sc.nodes[(size_t)sc.root_ref / 4];
  float u[12];
  for (int a = 0; a < 3; ++a) {
    u[2 * a] = pt_minf(b[2 * a], b[2 * a + 1]);
    u[6 + 2 * a] = pt_maxf(b[6 + 2 * a], b[6 + 2 * a + 1]);
  }
  float E, X;
  slab6(w, u, 0, E, X);
  if (pt_minf(X, w.closest) >= E) w.push((uint32_t)sc.root_ref, E);
}

}  // namespace

int main(int argc, char** argv) {
  const bool table_mode = argc == 13 && strcmp(argv[12], "table") == 0;
  if (argc != 12 && !table_mode) {
    fprintf(stderr, "usage: %s SHELL N_INNER ROOT_REF MAX_LEAF_DEPTH STACK nodes spheres quads tris rays out [table]\n",
            argv[0]);
    return 2;
  }
  Scene sc;
  sc.shell = atoi(argv[1]);
  sc.n_inner = atoi(argv[2]);
  sc.root_ref = atoi(argv[3]);
  sc.max_leaf_depth = atoi(argv[4]);
  const int32_t stack = atoi(argv[5]);
  std::vector<float> rays;
  if (!read_all_f32(argv[6], sc.nodes) || !read_all_f32(argv[7], sc.spheres) || !read_all_f32(argv[8], sc.quads) ||
      !read_all_f32(argv[9], sc.tris) || !read_all_f32(argv[10], rays)) {
    fprintf(stderr, "cannot read the inputs\n");
    return 2;
  }
  if (sc.n_inner < 0 || sc.nodes.size() < (size_t)sc.n_inner * (kChainNodeBytes / 4) || rays.size() % 7 != 0 ||
      sc.spheres.size() % 4 != 0 || sc.quads.size() % 16 != 0 || sc.tris.size() % 12 != 0) {
    fprintf(stderr, "input sizes do not fit\n");
    return 2;
  }
  const Load ld{&sc.nodes};
  const ShellChain ch = shell_chain_find(ld, sc.shell, sc.n_inner, sc.root_ref);
  const ShellPlan pl = shell_chain_plan(ch, stack, sc.max_leaf_depth);
  printf("chain m %d full %d side %u plan m %d skip %d slots %d off", ch.m, ch.full ? 1 : 0, ch.side, pl.m,
         pl.skip ? 1 : 0, pl.m ? shell_chain_slots(sc.max_leaf_depth, pl.m, pl.skip) : sc.max_leaf_depth + 1);
  for (int k = 0; k < ch.m; ++k) printf(" %u", ch.off[k]);
  printf("\n");

  // the shell's leaf box and sphere, as load_shell_box / load_shell_sphere read them
  float4 sph = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float* pbox = nullptr;
  int pc = 0;
  if (pl.m > 0) {
    const uint32_t v = (uint32_t)sc.shell - 1u;
    pc = (int)(v & 1u);
    pbox = &sc.nodes[(v & ~1u) / 4];
    const int32_t ref = (int32_t)pt_chain_u(pbox[12 + pc]);
    const size_t ix = (size_t)(ref & 0x01ffffff);
    if (ref >= 0 || ((ref >> 28) & 3) != kSphere || 4 * ix + 4 > sc.spheres.size()) {
      fprintf(stderr, "the hint does not point at a sphere leaf\n");
      return 2;
    }
    sph = f4(sc.spheres, 4 * ix);
  }

  // the wave's table: each entry computed where it is read, or (table mode)
  // built once into an array, lane by lane, as the megakernel's prologue does
  const SphereLoad sl{&sc.spheres};
  const ShellTableDirect<Load, SphereLoad> direct{ld, sl, ch, pl, sc.shell, sc.n_inner};
  uint32_t tab[128];
  for (int lane = 0; lane < 64; ++lane) {
    tab[lane] = shell_table_entry(ld, sl, ch, pl, sc.shell, sc.n_inner, lane);
    tab[64 + lane] = shell_table_entry(ld, sl, ch, pl, sc.shell, sc.n_inner, 64 + lane);
  }
  const TableLoad tl{tab};
  if (table_mode) {
    printf("table");
    for (int i = 0; i < kTabSize; ++i) printf(" %08x", tab[i]);
    printf("\n");
  }

  const size_t n = rays.size() / 7;
  std::vector<uint32_t> out(8 * n);
  bool overflow = false;
  Walk w;
  for (size_t r = 0; r < n; ++r) {
    const float* q = &rays[7 * r];
    const pt_v3 o = pt_v3f(q[0], q[1], q[2]), d = pt_v3f(q[3], q[4], q[5]);
    uint32_t* res = &out[8 * r];
    // the ordinary walk
    ray(w, o, d, q[6]);
    begin_root(sc, w);
    run(sc, w);
    overflow = overflow || w.overflow;
    res[0] = (uint32_t)w.best, res[1] = pt_chain_u(w.closest), res[2] = (uint32_t)w.peak;
    // the expanded walk: begin_segment and the shading round's finish (pt_megakernel.hip)
    ray(w, o, d, q[6]);
    bool gate = false, expanded = false, finished = false;
    if (pl.m > 0) {
      const float4 gs = table_mode ? make_float4(pt_chain_f(tab[kTabSphere]), pt_chain_f(tab[kTabSphere + 1]),
                                                 pt_chain_f(tab[kTabSphere + 2]), pt_chain_f(tab[kTabSphere + 3]))
                                   : sph;
      const pt_v3 oc = pt_sub(o, pt_v3f(gs.x, gs.y, gs.z));
      gate = 4.0f * pt_dot(oc, oc) <= gs.w * gs.w;
    }
    auto push = [&](uint32_t ref, float E) { w.push(ref, E); };
    if (gate)
      expanded = table_mode ? shell_chain_begin(tl, ch, pl, w.o, w.d, w.inv, w.tmin, w.closest, true, push)
                            : shell_chain_begin(direct, ch, pl, w.o, w.d, w.inv, w.tmin, w.closest, true, push);
    if (!expanded) begin_root(sc, w);
    run(sc, w);
    if (pl.skip && gate && w.best == 0) {  // shell_hit: the leaf's box, then its sphere
      finished = true;
      float E, X, t;
      if (table_mode) {  // shell_from_table: the leaf's box in the order lo x, y, z, hi x, y, z, its code and sphere
        float b[12];
        for (int a = 0; a < 6; ++a) b[2 * a] = b[2 * a + 1] = pt_chain_f(tab[kTabLeaf + a]);
        slab6(w, b, 0, E, X);
        const float4 ts = make_float4(pt_chain_f(tab[kTabSphere]), pt_chain_f(tab[kTabSphere + 1]),
                                      pt_chain_f(tab[kTabSphere + 2]), pt_chain_f(tab[kTabSphere + 3]));
        if (pt_minf(X, kTMax) >= E && hit_sphere_t<true>(ts, w.o, w.d, w.tmin, kTMax, t)) {
          w.closest = t;
          w.best = (int32_t)tab[kTabLeaf + 6];
        }
      } else {
        slab6(w, pbox, pc, E, X);
        if (pt_minf(X, kTMax) >= E && hit_sphere_t<true>(sph, w.o, w.d, w.tmin, kTMax, t)) {
          w.closest = t;
          w.best = (int32_t)pt_chain_u(pbox[12 + pc]);
        }
      }
    }
    overflow = overflow || w.overflow;
    res[3] = (uint32_t)w.best, res[4] = pt_chain_u(w.closest), res[5] = (uint32_t)w.peak;
    res[6] = expanded ? 1u : 0u, res[7] = finished ? 1u : 0u;
  }
  FILE* f = fopen(argv[11], "wb");
  if (!f || fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size() || fclose(f) != 0) {
    fprintf(stderr, "cannot write %s\n", argv[11]);
    return 2;
  }
  if (overflow) {
    fprintf(stderr, "a walk needed more than %d slots\n", kCap);
    return 1;
  }
  return 0;
}
