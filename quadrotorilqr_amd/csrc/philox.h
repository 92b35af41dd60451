// philox.h -- the counter-based generator of the Monte-Carlo kernels (monte_carlo_kernels.h): Philox4x32-10 (Salmon, Moraes, Dror and
// Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter and key this library gives it, and two unit normals from
// its four words.  A draw is a function of (seed, plan, sample, row, stream, pair) alone: not of B, S, the grid or the kernel, so any
// draw can be reproduced from its indices (tests/monte_carlo_numpy.py restates all of this in NumPy).
//
// Lane-local, no memory, no table: QILQR_HD like se3_math.h, and tests/host_monte_carlo_harness.cpp compiles the same text with g++.
// The sine and cosine are this file's own: the angle is reduced in TURNS, which is exact (t is a multiple of 2^-53, the quadrant a
// multiple of 1/4), and the remainder |x| <= pi/4 goes through the two minimax kernels of fdlibm (k_sin.c, k_cos.c; error below 1 ulp
// there).  A library sincos would bring its large-argument reduction along -- a table walk that costs scratch on the device -- for
// arguments that never leave [0, 2 pi); and with one text the host and the device differ in log and sqrt alone.
#pragma once

#include <math.h>
#include <stdint.h>

#include "se3_math.h"  // QILQR_HD

// every product and sum below is rounded where the source says so (the polynomials are written with fma)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace qilqr {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;  // the multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;  // the Weyl constants: golden ratio, sqrt(3) - 1
constexpr uint32_t MC_STREAM_GUSTS = 0, MC_STREAM_STATES = 1, MC_STREAM_CONTROLS = 2;

// c <- Philox4x32-10(c; k)
QILQR_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c[0], p1 = (uint64_t)PHILOX_M1 * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += PHILOX_W0; k1 += PHILOX_W1;
  }
}

// the four words of draw (seed; plan, sample, row, stream, pair): counter {row, sample, plan, stream << 16 | pair}, key {seed lo, seed hi}
QILQR_HD void mc_words(uint64_t seed, uint32_t plan, uint32_t sample, uint32_t row, uint32_t stream, uint32_t pair, uint32_t w[4]) {
  w[0] = row; w[1] = sample; w[2] = plan; w[3] = (stream << 16) | pair;
  philox4x32_10(w, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}

// sin and cos of 2 pi t for t in [0, 1): the quadrant k = round(4 t), the remainder r = t - k / 4 in [-1/8, 1/8] (exact), x = 2 pi r
// rounded once, then fdlibm's kernels on |x| <= pi / 4 and the quadrant's signs
QILQR_HD void mc_sincos_turns(double t, double &s, double &c) {
  const double k = floor(fma(4.0, t, 0.5));  // 0 .. 4
  const double r = fma(-0.25, k, t);
  const double x = 6.283185307179586476925286766559 * r, z = x * x;
  double ps = 1.58969099521155010221e-10;
  ps = fma(ps, z, -2.50507602534068634195e-08);
  ps = fma(ps, z, 2.75573137070700676789e-06);
  ps = fma(ps, z, -1.98412698298579493134e-04);
  ps = fma(ps, z, 8.33333333332248946124e-03);
  ps = fma(ps, z, -1.66666666666666324348e-01);
  const double sx = fma(x * z, ps, x);
  double pc = -1.13596475577881948265e-11;
  pc = fma(pc, z, 2.08757232129817482790e-09);
  pc = fma(pc, z, -2.75573143513906633035e-07);
  pc = fma(pc, z, 2.48015872894767294178e-05);
  pc = fma(pc, z, -1.38888888888741095749e-03);
  pc = fma(pc, z, 4.16666666666666019037e-02);
  const double cx = fma(z * z, pc, fma(-0.5, z, 1.0));
  const int q = (int)k & 3;
  const double a = (q & 1) ? cx : sx, b = (q & 1) ? sx : cx;  // sin(x + q pi/2), cos(x + q pi/2) up to sign
  s = (q & 2) ? -a : a;
  c = (q == 1 || q == 2) ? -b : b;
}

// two unit normals from four words (Box-Muller): u1 in (0, 1] from the top 53 bits of {w0, w1} (the logarithm is finite), t in [0, 1)
// from those of {w2, w3}.  All-zero words give (sqrt(106 ln 2), 0); all-one words give a zero in both (u1 = 1).
QILQR_HD void mc_normals(const uint32_t w[4], double &z0, double &z1) {
  const double two26 = 67108864.0, twom53 = 1.1102230246251565404236316680908203125e-16;
  const double a = (double)(w[0] >> 5) * two26 + (double)(w[1] >> 6);
  const double u1 = (a + 1.0) * twom53;
  const double t = ((double)(w[2] >> 5) * two26 + (double)(w[3] >> 6)) * twom53;
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
  mc_sincos_turns(t, s, c);
  z0 = r * c;
  z1 = r * s;
}

// the pair of normals of a draw
QILQR_HD void mc_draw(uint64_t seed, uint32_t plan, uint32_t sample, uint32_t row, uint32_t stream, uint32_t pair, double &z0, double &z1) {
  uint32_t w[4];
  mc_words(seed, plan, sample, row, stream, pair, w);
  mc_normals(w, z0, z1);
}

}  // namespace qilqr

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
