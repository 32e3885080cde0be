// pt_shell_chain.hpp — the enclosing medium shell's ancestor chain, expanded
// when a segment begins. Host and device: the megakernel's
// SHELL kernels call these functions (pt_megakernel.hip), and shell_chain_check.cpp
// runs them on the CPU against the ordinary walk.
//
// The shell's leaf box B is the box of every one of its ancestors (claim 2 of
// the hint, include/ptmi.h: everything else lies strictly inside B, so each
// union is B again, bit for bit). A ray that starts inside the shell is inside
// all of them, its entry distance into each is tmin, and the ordinary walk pops
// and expands them one dependent step after the other with nothing to cull.
// Level k of the chain is the ancestor at depth k: one child is the chain child
// (box B), the other the sibling subtree S_k. What the walk does with the chain
// depends on the ray only through one slab test and one near / far decision
// per sibling, so a segment can begin with all of it done:
//   * shell_chain_find: the chain, from the hint and the node array alone;
//   * shell_chain_plan: how many levels a kernel's stack allows (the bound);
//   * shell_table_entry: the wave's table, everything the begin and the
//     shading round's shell tests read, fetched once per wave and launch;
//   * shell_chain_begin: the stack the ordinary walk would reach, chain entries
//     left out, in the ordinary walk's pop order, from the table.
#pragma once
#include <stdint.h>

#include "../../include/ptmi_math.h"

namespace ptmi {

constexpr int kShellChainMax = 6;      // levels expanded at most
constexpr uint32_t kChainNodeBytes = 80;  // node stride (kNodeBytes, pt_device.hpp)

// Node floats (include/ptmi.h): [2 a + c] = box bound a of child c in the
// order min x, y, z, max x, y, z; [12 + c] its ref, [14 + c] its z centre.
struct ShellChain {
  uint32_t off[kShellChainMax];  // byte offset of level k's node
  uint32_t side;                 // bit k: the chain child of level k is child 1
  int32_t m;                     // levels found, 0: no expansion
  bool full;                     // level m - 1 is the hint's node: its chain child is the shell's leaf
};

PT_HD float pt_chain_f(uint32_t b) {
  union {
    uint32_t u;
    float f;
  } v;
  v.u = b;
  return v.f;
}
PT_HD uint32_t pt_chain_u(float f) {
  union {
    uint32_t u;
    float f;
  } v;
  v.f = f;
  return v.u;
}

// ld(off, i): the bits of float i of the node at byte offset off.
// The chain child of a level is the child whose six box floats and z centre
// are bit-equal to the shell leaf's as its parent stores them; above the
// hint's node it must be internal. The walk stops at the hint's node, after
// kShellChainMax levels, when no child or both children match, or at an
// offset outside the n_inner nodes.
template <class L>
PT_HD ShellChain shell_chain_find(const L& ld, int32_t shell, int32_t n_inner, int32_t root_ref) {
  ShellChain ch{};
  if (shell <= 0 || n_inner <= 0 || root_ref < 0) return ch;
  const uint32_t v = (uint32_t)shell - 1u, pc = v & 1u, poff = v & ~1u;
  const uint32_t end = (uint32_t)n_inner * kChainNodeBytes;
  if (poff >= end) return ch;
  uint32_t box[7];
#pragma unroll
  for (int a = 0; a < 7; ++a) box[a] = ld(poff, 2u * (uint32_t)a + pc + (a == 6 ? 2u : 0u));  // a = 6: the z centre
  uint32_t cur = (uint32_t)root_ref;
  bool go = true;
#pragma unroll
  for (int k = 0; k < kShellChainMax; ++k) {
    if (go) {
      go = false;
      if (cur < end) {
        bool m0 = true, m1 = true;
#pragma unroll
        for (int a = 0; a < 7; ++a) {
          const uint32_t i = 2u * (uint32_t)a + (a == 6 ? 2u : 0u);
          m0 = m0 && ld(cur, i) == box[a];
          m1 = m1 && ld(cur, i + 1u) == box[a];
        }
        if (m0 != m1) {
          const uint32_t c = m1 ? 1u : 0u;
          const int32_t ref = (int32_t)ld(cur, 12u + c);
          if (cur == poff) {
            if (c == pc) {  // the hint's node: the chain ends on the shell's leaf
              ch.off[k] = cur;
              ch.side |= c << k;
              ch.m = k + 1;
              ch.full = true;
            }
          } else if (ref >= 0) {
            ch.off[k] = cur;
            ch.side |= c << k;
            ch.m = k + 1;
            cur = (uint32_t)ref;
            go = true;
          }
        }
      }
    }
  }
  return ch;
}

// Stack slots. The ordinary walk pops a node of depth d with at most d entries
// below it, so it needs max_leaf_depth + 1 slots. With m levels expanded, the
// near sibling S_k (root depth k + 1, leaves at most max_leaf_depth - k - 1
// below its root) is popped above the other m - 1 siblings and, unless the
// shell's leaf is skipped, the rest of the chain: (m - 1) + rest below, then
// max_leaf_depth - k slots for its own walk, most at k = 0. The rest of the
// chain, a node of depth m, is popped above far siblings only, at most m; from
// there the walk is the ordinary one.
PT_HD int32_t shell_chain_slots(int32_t max_leaf_depth, int32_t m, bool skip) {
  return max_leaf_depth + m - (skip ? 1 : 0);
}

struct ShellPlan {
  int32_t m;  // levels to expand (0: the ordinary begin)
  bool skip;  // the shell's leaf is not pushed: a segment that hits nothing else tests it when it is shaded
};

// The levels a stack of `stack` slots allows.
PT_HD ShellPlan shell_chain_plan(const ShellChain& ch, int32_t stack, int32_t max_leaf_depth) {
  ShellPlan p{0, false};
  if (ch.m < 1) return p;
  if (ch.full && shell_chain_slots(max_leaf_depth, ch.m, true) <= stack) {
    p.m = ch.m;
    p.skip = true;
    return p;
  }
  const int32_t fit = stack - max_leaf_depth;  // shell_chain_slots(mld, m, false) <= stack
  p.m = ch.m < fit ? ch.m : fit;
  if (p.m < 1) p.m = 0;
  return p;
}

// The stack slots the host asks for on behalf of a scene with a hint: room for
// kShellChainMax - 1 levels with the leaf skipped, on a rung that has SHELL
// kernels (16, 17, 18, 20: pt_megakernel.hip), never more than 20 and never
// fewer than the ordinary walk needs.
#ifndef PTMI_SHELL_CHAIN_EXTRA
#define PTMI_SHELL_CHAIN_EXTRA (kShellChainMax - 2)  // A/B on MI355X, C2: DESIGN.md §12a
#endif
PT_HD int32_t shell_chain_stack_request(int32_t stack_needed) {
  if (stack_needed > 20) return stack_needed;
  int32_t want = stack_needed + PTMI_SHELL_CHAIN_EXTRA;
  if (want >= 19) want = 20;
  return want;
}

// The wave-resident table: everything the expanded begin and
// the shading round's shell tests read, in canonical form, so that a reader
// needs neither a node offset nor a side bit. Dword i:
//   kTabShared + j              the shared box (the chain child of level 0)
//   kTabLevel + 10 k + j        the sibling of level k < p.m
//     j = 0..5  box floats min x, y, z, max x, y, z
//     j = 6, 7  cx, cy = (lo + hi) * 0.5f, node_step's expression
//     j = 8     cz as the node stores it
//     j = 9     the sibling's ref (levels only)
//   kTabRest                    the chain child's ref of level p.m - 1
//   kTabLeaf + 0..5, + 6        the shell's leaf box as its parent stores it, its leaf code
//   kTabSphere + 0..3           the shell's sphere {c.xyz, R}
// Entries of levels not expanded are 0; without a plan (p.m == 0) only the
// leaf and sphere entries are filled. The megakernel keeps the table in two
// VGPRs (lane i: dwords i and 64 + i), built once per wave and launch from the
// node array, so it follows a device refit; shell_chain_check.cpp keeps it in
// an array.
constexpr int kTabShared = 0;
constexpr int kTabLevel = 9;
constexpr int kTabLevelStride = 10;
constexpr int kTabRest = kTabLevel + kTabLevelStride * kShellChainMax;
constexpr int kTabLeaf = kTabRest + 1;
constexpr int kTabSphere = kTabLeaf + 7;
constexpr int kTabSize = kTabSphere + 4;
static_assert(kTabSize <= 128, "the table fits two dwords per lane");

// Dword i of the table. ld(off, i) as above; sph(ref, a): the bits of float a
// of the sphere that leaf code ref names, 0 if ref is not a sphere leaf (a
// wrong hint reads nothing out of bounds). i may differ from lane to lane: one
// or two loads per entry.
template <class L, class S>
PT_HD uint32_t shell_table_entry(const L& ld, const S& sph, const ShellChain& ch, const ShellPlan& p, int32_t shell,
                                 int32_t n_inner, int i) {
  if (i < 0 || i >= kTabSize) return 0u;
  if (i <= kTabRest) {
    if (p.m < 1) return 0u;
    int k = 0, j = i;
    bool chain_child = true;
    if (i == kTabRest) {
      k = p.m - 1;
      j = 9;
    } else if (i >= kTabLevel) {
      k = (i - kTabLevel) / kTabLevelStride;
      j = (i - kTabLevel) - kTabLevelStride * k;
      chain_child = false;
      if (k >= p.m) return 0u;
    }
    // selects on values, written out: an index that varies by lane would put the chain in scratch memory
    static_assert(kShellChainMax == 6, "one select per level");
    const uint32_t o0 = ch.off[0], o1 = ch.off[1], o2 = ch.off[2], o3 = ch.off[3], o4 = ch.off[4], o5 = ch.off[5];
    const uint32_t off = k == 0 ? o0 : k == 1 ? o1 : k == 2 ? o2 : k == 3 ? o3 : k == 4 ? o4 : o5;
    const uint32_t c = ((ch.side >> k) & 1u) ^ (chain_child ? 0u : 1u);
    if (j < 6) return ld(off, 2u * (uint32_t)j + c);
    if (j < 8) {
      const uint32_t a = 2u * (uint32_t)(j - 6) + c;
      return pt_chain_u((pt_chain_f(ld(off, a)) + pt_chain_f(ld(off, a + 6u))) * 0.5f);
    }
    return ld(off, (j == 8 ? 14u : 12u) + c);
  }
  if (shell <= 0 || n_inner <= 0) return 0u;
  const uint32_t v = (uint32_t)shell - 1u, pc = v & 1u, poff = v & ~1u;
  if (poff >= (uint32_t)n_inner * kChainNodeBytes) return 0u;
  if (i < kTabSphere) {
    const int j = i - kTabLeaf;
    return ld(poff, (j < 6 ? 2u * (uint32_t)j : 12u) + pc);
  }
  return sph((int32_t)ld(poff, 12u + pc), i - kTabSphere);
}

// A table loader that computes each entry from the node array where it is
// read: the reference for the table kept in registers or in an array.
template <class L, class S>
struct ShellTableDirect {
  const L& ld;
  const S& sph;
  const ShellChain& ch;
  const ShellPlan& p;
  int32_t shell, n_inner;
  PT_HD uint32_t operator()(int i) const { return shell_table_entry(ld, sph, ch, p, shell, n_inner, i); }
};

// The expanded begin of a segment (o, d, inv, tmin; closest = tmax) with
// p.m >= 1 levels, from the table: tl(i) is dword i. Written to run converged:
// every lane computes, a lane with `on` clear pushes nothing and gets false
// (the megakernel reads the table across lanes, which needs all of them
// active: DESIGN.md §4). False for a lane with `on` set: the shared box fails
// its slab test, nothing was pushed and the caller begins at the root as
// usual. push(ref, E) stores one
// entry on top of the stack. (A/B on MI355X, not kept: every entry stored at
// the top and the top moved only for a kept one, as node_step does, instead of
// a branch per entry: C2 -1.8 %, profiles/chain/bench_parent_vs_new.json.)
// E, X and the projected centre distances are node_step's expressions
// (pt_device.hpp) on the same floats, so each entry {ref, E} has the bits the
// ordinary walk would have stored, and near / far is its `ln` (a tie goes to
// child 1). Order, bottom to top: the far siblings in increasing k, the rest
// of the chain (the chain child of level m - 1 with the shared box's E) unless
// skipped, the near siblings in decreasing k: the ordinary walk's pop order.
template <class T, class P>
PT_HD bool shell_chain_begin(const T& tl, const ShellChain& ch, const ShellPlan& p, pt_v3 o, pt_v3 d, pt_v3 inv,
                             float tmin, float tmax, bool on, P&& push) {
  auto slab1 = [&](int b, float& E, float& X, float& dist) {
    const float lox = pt_chain_f(tl(b + 0)), loy = pt_chain_f(tl(b + 1)), loz = pt_chain_f(tl(b + 2));
    const float hix = pt_chain_f(tl(b + 3)), hiy = pt_chain_f(tl(b + 4)), hiz = pt_chain_f(tl(b + 5));
    const float cx = pt_chain_f(tl(b + 6)), cy = pt_chain_f(tl(b + 7)), cz = pt_chain_f(tl(b + 8));
    const float t0x = (lox - o.x) * inv.x, t1x = (hix - o.x) * inv.x;
    const float t0y = (loy - o.y) * inv.y, t1y = (hiy - o.y) * inv.y;
    const float t0z = (loz - o.z) * inv.z, t1z = (hiz - o.z) * inv.z;
    E = pt_maxf(pt_maxf(pt_minf(t0x, t1x), pt_minf(t0y, t1y)), pt_maxf(pt_minf(t0z, t1z), tmin));
    X = pt_minf(pt_minf(pt_maxf(t0x, t1x), pt_maxf(t0y, t1y)), pt_maxf(t0z, t1z));
    dist = ((cx - o.x) * d.x + (cy - o.y) * d.y) + (cz - o.z) * d.z;
  };
  float Eg, Xg, dg;
  slab1(kTabShared, Eg, Xg, dg);
  const bool ex = on && pt_minf(Xg, tmax) >= Eg;
  const uint32_t rest = tl(kTabRest);  // read here, not under the lane's own `ex`
  uint32_t ref[kShellChainMax];
  float E[kShellChainMax];
  bool far_[kShellChainMax], near_[kShellChainMax];
#pragma unroll
  for (int k = 0; k < kShellChainMax; ++k) {
    far_[k] = near_[k] = false;
    ref[k] = 0u;
    E[k] = 0.0f;
    if (k < p.m) {
      const uint32_t s = ((ch.side >> k) & 1u) ^ 1u;
      float X, ds;
      slab1(kTabLevel + kTabLevelStride * k, E[k], X, ds);
      ref[k] = tl(kTabLevel + kTabLevelStride * k + 9);
      const bool hit = ex && X >= E[k];
      const bool nr = s == 0u ? ds < dg : !(dg < ds);  // ln: child 0 is near iff dist0 < dist1
      near_[k] = hit && nr;
      far_[k] = hit && !nr;
    }
  }
#pragma unroll
  for (int k = 0; k < kShellChainMax; ++k)
    if (far_[k]) push(ref[k], E[k]);
  if (ex && !p.skip) push(rest, Eg);
#pragma unroll
  for (int k = kShellChainMax - 1; k >= 0; --k)
    if (near_[k]) push(ref[k], E[k]);
  return ex;
}

}  // namespace ptmi
