// update_check.cpp — the scene update's arithmetic (pt_update_math.hpp, the
// functions the kernels of pt_update.hip call) run on the CPU: a stand-alone
// host program, no HIP, no GPU. `make update_check` builds it;
// tests/test_update_abi.py compares its output with the numpy reference bit for
// bit.
//
//   update_check MODE in.f32 out.f32
//
// in.f32 is raw little-endian f32, a whole number of records:
//   sphere  4 per record {c.xyz, r}            -> 6 {mn.xyz, mx.xyz}
//   quad    9 per record {Q, u, v}             -> 6
//   tri     9 per record {v0, v1, v2}          -> 6
//   union  12 per record {l.mn, l.mx, r.mn, r.mx} -> 12 {mn, mx of the union,
//          centre.xyz of l, centre.xyz of r}
// Exit 0 on success, 2 on bad arguments or I/O.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pt_check_io.hpp"
#include "pt_update_math.hpp"

using namespace ptmi;

static void put_box(std::vector<float>& out, const UpdBox& b) {
  out.insert(out.end(), b.mn, b.mn + 3);
  out.insert(out.end(), b.mx, b.mx + 3);
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s sphere|quad|tri|union in.f32 out.f32\n", argv[0]);
    return 2;
  }
  const char* mode = argv[1];
  const size_t rec = !strcmp(mode, "sphere") ? 4 : !strcmp(mode, "quad") || !strcmp(mode, "tri") ? 9
                     : !strcmp(mode, "union") ? 12 : 0;
  if (!rec) {
    fprintf(stderr, "unknown mode %s\n", mode);
    return 2;
  }
  std::vector<float> in, out;
  if (!read_all_f32(argv[2], in) || in.size() % rec) {
    fprintf(stderr, "cannot read whole records of %zu f32\n", rec);
    return 2;
  }
  for (size_t i = 0; i < in.size(); i += rec) {
    const float* r = in.data() + i;
    if (rec == 4) {
      put_box(out, upd_sphere_box(r));
    } else if (rec == 9) {
      put_box(out, mode[0] == 'q' ? upd_quad_box(r) : upd_tri_box(r));
    } else {
      UpdBox a, b;
      for (int k = 0; k < 3; ++k) {
        a.mn[k] = r[k];
        a.mx[k] = r[3 + k];
        b.mn[k] = r[6 + k];
        b.mx[k] = r[9 + k];
      }
      put_box(out, upd_union(a, b));
      for (int k = 0; k < 3; ++k) out.push_back(upd_centre(a, k));
      for (int k = 0; k < 3; ++k) out.push_back(upd_centre(b, k));
    }
  }
  if (!write_f32(argv[3], out)) {
    fprintf(stderr, "cannot write the output\n");
    return 2;
  }
  return 0;
}
