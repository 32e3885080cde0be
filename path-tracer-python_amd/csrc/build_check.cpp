// build_check.cpp — the device builder and packer (pt_build_math.hpp, the
// per-lane phases the kernels of pt_build.hip call) run on the CPU in the
// kernels' order: a stand-alone host program, no HIP, no GPU. Each phase runs
// for lane 0 .. 1023 in a plain loop where the kernel has a barrier. `make
// build_check` builds it; tests/test_build_abi.py compares its output with the
// host builder and with pack_device bit for bit.
//
//   build_check DIR
//
// reads DIR/spheres.f32, quads.f32, tris.f32 (builder-form records of 4, 9 and
// 9 f32; a missing file is no primitive of that type) and writes the seven
// arrays DIR/out_{bmin,bmax,left,right,parent,ptype,pidx} and out_status. If
// DIR/mats.f32 exists it also reads the scene's device rows rows_{s,t,q}.f32,
// mats.f32 and the maps old_{s,t,q}.i32 (reference index -> old device row)
// and writes out_nodes, out_ref_nodes, out_rows_{s,t,q}, out_mats,
// out_new_{s,t,q}, out_perm_{s,t,q} and out_info. An optional DIR/poke.i32
// holds triples (array, node, value) written into the built arrays between the
// build and the pack (array 0 left, 1 right, 2 parent, 3 prim_type, 4
// prim_idx): a tree the pack has to reject. Files are raw little-endian
// 4-byte words. It prints the status block, the two fallback counts among them.
// Exit 0 on success, 2 on bad arguments or I/O.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "pt_build_math.hpp"
#include "pt_check_io.hpp"

using namespace ptmi;

#define BUILD_CHECK_EACH(x) \
  for (int lane = 0; lane < kBuildLanes; ++lane) { x; }

static std::string g_dir;

static bool exists(const char* name) {
  FILE* f = fopen((g_dir + "/" + name).c_str(), "rb");
  if (f) fclose(f);
  return f != nullptr;
}

// The words of a file as they are (an i32 file read as f32 keeps its bits); a missing file is empty.
static bool load(const char* name, std::vector<float>& v, size_t row_words) {
  if (!exists(name)) return true;
  if (!read_all_f32((g_dir + "/" + name).c_str(), v) || v.size() % row_words) {
    fprintf(stderr, "%s: not whole rows of %zu words\n", name, row_words);
    return false;
  }
  return true;
}

static bool save(const char* name, const void* p, size_t words) {
  std::vector<float> v(words);
  if (words) memcpy(v.data(), p, 4 * words);
  if (!write_f32((g_dir + "/" + name).c_str(), v)) {
    fprintf(stderr, "cannot write %s\n", name);
    return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s DIR\n", argv[0]);
    return 2;
  }
  g_dir = argv[1];
  std::vector<float> sph, quads, tris;
  if (!load("spheres.f32", sph, 4) || !load("quads.f32", quads, 9) || !load("tris.f32", tris, 9)) return 2;
  const int64_t n64 = (int64_t)(sph.size() / 4 + quads.size() / 9 + tris.size() / 9);
  if (n64 > PTMI_BUILD_MAX_PRIMS) {
    fprintf(stderr, "%lld primitives, at most %d\n", (long long)n64, PTMI_BUILD_MAX_PRIMS);
    return 2;
  }
  const int32_t n = (int32_t)n64, nn = n ? 2 * n - 1 : 0;
  std::vector<float> bmin(3 * (size_t)nn), bmax(3 * (size_t)nn);
  std::vector<int32_t> left(nn), right(nn), parent(nn), ptype(nn), pidx(nn), status(PTMI_BUILD_STATUS_WORDS, -1);
  std::vector<char> work(build_workspace_bytes(n) + 16);
  BuildCtx c = {};
  c.in = {sph.data(), quads.data(), tris.data(), (int32_t)(sph.size() / 4), (int32_t)(quads.size() / 9),
          (int32_t)(tris.size() / 9)};
  c.out = {bmin.data(), bmax.data(), left.data(), right.data(), parent.data(), ptype.data(), pidx.data(), status.data()};
  c.n = n;
  if (n) build_carve(n, work.data(), &c.ws);
  BuildShared* shp = new BuildShared();
  BuildShared& sh = *shp;
  {
    PTMI_BUILD_LEVELS(BUILD_CHECK_EACH, sh, c)
    build_finish(c, sh, level);
  }
  printf("status=%d n_nodes=%d levels=%d max_leaf_depth=%d fallback_a=%d fallback_b=%d\n", status[0], status[1],
         status[2], status[3], status[4], status[5]);
  bool ok = save("out_bmin", bmin.data(), bmin.size()) && save("out_bmax", bmax.data(), bmax.size()) &&
            save("out_left", left.data(), nn) && save("out_right", right.data(), nn) &&
            save("out_parent", parent.data(), nn) && save("out_ptype", ptype.data(), nn) &&
            save("out_pidx", pidx.data(), nn) && save("out_status", status.data(), status.size());
  if (ok && exists("mats.f32") && n) {
    // by type code: spheres, triangles, quads
    const int32_t counts[3] = {c.in.ns, c.in.nt, c.in.nq};
    static const char* const tag[3] = {"s", "t", "q"};
    std::vector<float> rows[3], mats, oldw[3], nodes(kPackNodeFloats * (size_t)(n - 1)), refn(kPackRefFloats * (size_t)nn);
    std::vector<int32_t> newr[3], perm[3], info(PTMI_BUILD_INFO_WORDS, -1);
    PackCtx p = {};
    for (int t = 0; t < 3; ++t) {
      const std::string r = std::string("rows_") + tag[t] + ".f32", o = std::string("old_") + tag[t] + ".i32";
      if (!load(r.c_str(), rows[t], (size_t)pack_row_floats(t)) || !load(o.c_str(), oldw[t], 1)) return 2;
      if (rows[t].size() != (size_t)counts[t] * pack_row_floats(t) || oldw[t].size() != (size_t)counts[t]) {
        fprintf(stderr, "%s or %s: not one entry per primitive\n", r.c_str(), o.c_str());
        return 2;
      }
      newr[t].assign(counts[t], -1);
      perm[t].assign(counts[t], -1);
      p.counts[t] = counts[t];
      p.rows[t] = rows[t].data();
      p.old_row[t] = (const int32_t*)oldw[t].data();
      p.new_row[t] = newr[t].data();
      p.perm[t] = perm[t].data();
    }
    if (!load("mats.f32", mats, kPackMatFloats) || mats.size() != (size_t)n * kPackMatFloats) {
      fprintf(stderr, "mats.f32: not one row per primitive\n");
      return 2;
    }
    p.mat_base[0] = 0, p.mat_base[2] = counts[0], p.mat_base[1] = counts[0] + counts[2];
    p.nodes = nodes.data(), p.ref_nodes = refn.data(), p.mats = mats.data();
    p.built = c.out;
    p.info = info.data();
    p.n_prims = n, p.n = nn;
    std::vector<float> poke;
    if (!load("poke.i32", poke, 3)) return 2;
    for (size_t k = 0; k + 2 < poke.size(); k += 3) {
      int32_t w[3];
      memcpy(w, poke.data() + k, sizeof w);
      int32_t* const dst[5] = {left.data(), right.data(), parent.data(), ptype.data(), pidx.data()};
      if (w[0] < 0 || w[0] > 4 || w[1] < 0 || w[1] >= nn) {
        fprintf(stderr, "poke.i32: no such array or node\n");
        return 2;
      }
      dst[w[0]][w[1]] = w[2];
    }
    std::vector<char> pwork(build_workspace_bytes(n) + 16);
    pack_carve(p.counts, pwork.data(), &p.ws);
    if (status[0] != 0 || status[1] != nn) {
      pack_refuse(p, PTMI_BUILD_PACK_SKIPPED);
    } else {
      BUILD_CHECK_EACH(pack_begin(sh, lane));
      BUILD_CHECK_EACH(pack_copy(p, sh, lane, kBuildLanes));
      for (int which = 0; which < 2; ++which) {
        BUILD_CHECK_EACH(pack_count(p, sh, which, lane));
        for (int d = 1, row = 0; d < kBuildLanes; d <<= 1, row ^= 1) BUILD_CHECK_EACH(build_scan_step(sh, lane, d, row));
        BUILD_CHECK_EACH(pack_count_finish(p, sh, which, lane, kBuildLanes));
      }
      if (sh.status != 0) {
        pack_refuse(p, sh.status);
      } else {
        BUILD_CHECK_EACH(pack_leaves(p, lane, kBuildLanes));
        BUILD_CHECK_EACH(pack_nodes(p, status[3], lane, kBuildLanes));
      }
    }
    printf("pack=%d\n", info[10]);
    ok = save("out_nodes", nodes.data(), nodes.size()) && save("out_ref_nodes", refn.data(), refn.size()) &&
         save("out_mats", mats.data(), mats.size()) && save("out_info", info.data(), info.size());
    for (int t = 0; t < 3 && ok; ++t)
      ok = save((std::string("out_rows_") + tag[t]).c_str(), rows[t].data(), rows[t].size()) &&
           save((std::string("out_new_") + tag[t]).c_str(), newr[t].data(), newr[t].size()) &&
           save((std::string("out_perm_") + tag[t]).c_str(), perm[t].data(), perm[t].size());
  }
  delete shp;
  return ok ? 0 : 2;
}
