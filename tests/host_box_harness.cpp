// host_box_harness.cpp -- CPU test harness (tests only, never part of the product library): the box QP of the thrust-limit
// extension (quadrotorilqr_amd/csrc/box_qp.h) compiled with g++, for tests/test_control_limits_cpu.py.
#include "../quadrotorilqr_amd/csrc/box_qp.h"

using namespace qilqr;

extern "C" {
// H[16] (symmetric), g[4], l[4], h[4], Qux[4 x 12] row-major -> k[4], K[4 x 12] row-major, clamped (4-bit mask); returns 1, 0 if FAILED
int hb_box_qp(const double *H, const double *g, const double *l, const double *h, const double *Qux, double *k, double *K, int *clamped) {
  unsigned c = 0;
  BoxLdl f;
  const bool ok = box_qp(H, g, l, h, k, c, f);
  *clamped = (int)c;
  if (!ok) return 0;
  for (int j = 0; j < 12; ++j) {
    const double col[4] = {Qux[0 * 12 + j], Qux[1 * 12 + j], Qux[2 * 12 + j], Qux[3 * 12 + j]};
    double kc[4];
    box_gain_column(f, c, col, kc);
    for (int a = 0; a < 4; ++a) K[a * 12 + j] = kc[a];
  }
  return 1;
}
}
