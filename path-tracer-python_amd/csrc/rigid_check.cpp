// rigid_check.cpp — the rigid-body pose ABI's arithmetic (pt_rigid_math.hpp,
// the functions the kernel of pt_rigid.hip calls) run on the CPU: a stand-alone
// host program, no HIP, no GPU. `make rigid_check` builds it;
// tests/test_rigid_check.py compares its output with the Python definition
// (ptmi/rigid.py) bit for bit.
//
//   rigid_check MODE in.f64 out.f32
//
// in.f64 is raw little-endian f64, a whole number of records: a body of
// include/ptmi_rigid.h (15: R row-major, c, c'), then the rest record, then the
// row floats the kernel keeps, as f64:
//   sphere  15 + 3 {c} + 1 {r}                  -> 9 f32 {c.xyz, mn.xyz, mx.xyz}
//   quad    15 + 15 {Q, u, v, normal, w}        -> 22 f32 {the row, mn.xyz, mx.xyz}
//   tri     15 + 18 {v0, v1, v2, e1, e2, n}     -> 18 f32 {the row, mn.xyz, mx.xyz}
// Exit 0 on success, 2 on bad arguments or I/O.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pt_check_io.hpp"
#include "pt_rigid_math.hpp"

using namespace ptmi;

static bool read_all_f64(const char* path, std::vector<double>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  double buf[512];
  size_t got;
  while ((got = fread(buf, sizeof(double), 512, f)) > 0) v.insert(v.end(), buf, buf + got);
  const bool whole = feof(f) && ftell(f) % (long)sizeof(double) == 0;
  fclose(f);
  return whole;
}

static void put_box(std::vector<float>& out, const UpdBox& b) {
  out.insert(out.end(), b.mn, b.mn + 3);
  out.insert(out.end(), b.mx, b.mx + 3);
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s sphere|quad|tri in.f64 out.f32\n", argv[0]);
    return 2;
  }
  const char* mode = argv[1];
  const size_t B = kRigidBodyDoubles;
  const size_t rec = !strcmp(mode, "sphere") ? B + 4 : !strcmp(mode, "quad") ? B + 15 : !strcmp(mode, "tri") ? B + 18 : 0;
  if (!rec) {
    fprintf(stderr, "unknown mode %s\n", mode);
    return 2;
  }
  std::vector<double> in;
  std::vector<float> out;
  if (!read_all_f64(argv[2], in) || in.size() % rec) {
    fprintf(stderr, "cannot read whole records of %zu f64\n", rec);
    return 2;
  }
  for (size_t i = 0; i < in.size(); i += rec) {
    const double* body = in.data() + i;
    const double* r = body + B;
    if (rec == B + 4) {
      float row[4] = {0.0f, 0.0f, 0.0f, (float)r[3]};
      const UpdBox b = rigid_sphere(r, body, row);
      out.insert(out.end(), row, row + 3);
      put_box(out, b);
    } else if (rec == B + 15) {
      float row[16] = {0.0f};
      const UpdBox b = rigid_quad(r, body, row);
      out.insert(out.end(), row, row + 16);
      put_box(out, b);
    } else {
      float row[12] = {0.0f};
      const UpdBox b = rigid_tri(r, body, row);
      out.insert(out.end(), row, row + 12);
      put_box(out, b);
    }
  }
  if (!write_f32(argv[3], out)) {
    fprintf(stderr, "cannot write the output\n");
    return 2;
  }
  return 0;
}
