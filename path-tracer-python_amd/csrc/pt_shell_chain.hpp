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
//   * shell_chain_begin: the stack the ordinary walk would reach, chain entries
//     left out, in the ordinary walk's pop order.
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

// The expanded begin of a segment (o, d, inv, tmin; closest = tmax) with
// p.m >= 1 levels. False: the shared box fails its slab test, nothing was
// pushed and the caller begins at the root as usual. push(ref, E) stores one
// entry on top of the stack. (A/B on MI355X, not kept: every entry stored at
// the top and the top moved only for a kept one, as node_step does, instead of
// a branch per entry: C2 -1.8 %, profiles/chain/bench_parent_vs_new.json.)
// E, X and the projected centre distances are node_step's expressions
// (pt_device.hpp) on the same floats, so each entry {ref, E} has the bits the
// ordinary walk would have stored, and near / far is its `ln` (a tie goes to
// child 1). Order, bottom to top: the far siblings in increasing k, the rest
// of the chain (the chain child of level m - 1 with the shared box's E) unless
// skipped, the near siblings in decreasing k: the ordinary walk's pop order.
template <class L, class P>
PT_HD bool shell_chain_begin(const L& ld, const ShellChain& ch, const ShellPlan& p, pt_v3 o, pt_v3 d, pt_v3 inv,
                             float tmin, float tmax, P&& push) {
  auto slab1 = [&](uint32_t off, uint32_t c, float& E, float& X, float& dist) {
    const float lox = pt_chain_f(ld(off, 0u + c)), loy = pt_chain_f(ld(off, 2u + c)), loz = pt_chain_f(ld(off, 4u + c));
    const float hix = pt_chain_f(ld(off, 6u + c)), hiy = pt_chain_f(ld(off, 8u + c)), hiz = pt_chain_f(ld(off, 10u + c));
    const float cz = pt_chain_f(ld(off, 14u + c));
    const float t0x = (lox - o.x) * inv.x, t1x = (hix - o.x) * inv.x;
    const float t0y = (loy - o.y) * inv.y, t1y = (hiy - o.y) * inv.y;
    const float t0z = (loz - o.z) * inv.z, t1z = (hiz - o.z) * inv.z;
    E = pt_maxf(pt_maxf(pt_minf(t0x, t1x), pt_minf(t0y, t1y)), pt_maxf(pt_minf(t0z, t1z), tmin));
    X = pt_minf(pt_minf(pt_maxf(t0x, t1x), pt_maxf(t0y, t1y)), pt_maxf(t0z, t1z));
    const float cx = (lox + hix) * 0.5f, cy = (loy + hiy) * 0.5f;
    dist = ((cx - o.x) * d.x + (cy - o.y) * d.y) + (cz - o.z) * d.z;
  };
  float Eg, Xg, dg;
  slab1(ch.off[0], ch.side & 1u, Eg, Xg, dg);
  if (!(pt_minf(Xg, tmax) >= Eg)) return false;
  uint32_t ref[kShellChainMax];
  float E[kShellChainMax];
  bool far_[kShellChainMax], near_[kShellChainMax];
  uint32_t rest = 0u;
#pragma unroll
  for (int k = 0; k < kShellChainMax; ++k) {
    far_[k] = near_[k] = false;
    ref[k] = 0u;
    E[k] = 0.0f;
    if (k < p.m) {
      const uint32_t c = (ch.side >> k) & 1u, s = c ^ 1u;
      float X, ds;
      slab1(ch.off[k], s, E[k], X, ds);
      ref[k] = ld(ch.off[k], 12u + s);
      const bool hit = X >= E[k];
      const bool nr = s == 0u ? ds < dg : !(dg < ds);  // ln: child 0 is near iff dist0 < dist1
      near_[k] = hit && nr;
      far_[k] = hit && !nr;
      if (k == p.m - 1) rest = ld(ch.off[k], 12u + c);
    }
  }
#pragma unroll
  for (int k = 0; k < kShellChainMax; ++k)
    if (far_[k]) push(ref[k], E[k]);
  if (!p.skip) push(rest, Eg);
#pragma unroll
  for (int k = kShellChainMax - 1; k >= 0; --k)
    if (near_[k]) push(ref[k], E[k]);
  return true;
}

}  // namespace ptmi
