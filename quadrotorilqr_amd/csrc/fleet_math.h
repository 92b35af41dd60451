// fleet_math.h -- the arithmetic and the decisions of fleet deconfliction, stated once for the kernels of fleet.hip
// (fleet_kernels.h) and for the host program tests/host_fleet_harness.cpp, which agree bit for bit because both compile this text:
//   fleet_d2, fleet_pair_step   a pair's squared distance at a knot and its running minimum over the knots
//   fleet_before, FleetList     the total order (d2, partner row) and a sorted list of the K smallest under it
//   FleetBest                   what the summary keeps of ALL partners: the closest one and the number in conflict
//   fleet_fit                   a vehicle's constant-velocity line through its knots, least squares, with its residual
//   fleet_select_write          an ego's outputs from its merged list, its FleetBest and the fits
//   bob_row_kept, bob_set_problem   the row rule of qilqr_set_batch_obstacles_device and one problem's rows into the tiled table
// Every routine is lane-local.  One rounding per operation written: contraction is off, and every fused operation is an explicit fma.
// Squares decide: a distance is compared with `range` and `conflict` as d2 < range^2 and d2 < conflict^2, the squares rounded once
// (fleet_square); sqrt appears only in words that are reported (a distance, a residual), never in a decision.
#pragma once

#include <math.h>
#include <stdint.h>

#include "obstacles.h"  // OB_BWORDS, OB_TILE, bob_index
#include "se3_math.h"   // QILQR_HD

// (hipcc: the pragma; g++, which has no such pragma: the host program is built with -ffp-contract=off, tests/fleet_cases.py)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace qilqr {

constexpr int FLEET_MAX_NEIGHBOURS = 16;  // QILQR_FLEET_MAX_NEIGHBOURS
constexpr int FLEET_NBR = 4;              // QILQR_FLEET_NBR: partner row, distance, knot, the partner's fit residual
constexpr int FLEET_SUMMARY = 8;          // QILQR_FLEET_SUMMARY
constexpr unsigned FLEET_COVER = 1u, FLEET_YIELD_TO_LOWER = 2u;
constexpr int FLEET_FIT = 8;              // words of a vehicle's fit in the handle's scratch: c[3], v[3], residual, 1.0 if all of them are finite
constexpr int FLEET_NO_ROW = 0x7fffffff;  // the row of an empty list entry: behind every real row in the order

QILQR_HD double fleet_inf() { return HUGE_VAL; }
QILQR_HD double fleet_square(double x) { return x * x; }
QILQR_HD bool fleet_finite(double x) { return x - x == 0.0; }  // (neither NaN nor an infinity; no libm call in a decision)

// the squared distance of ego a and partner b at one knot
QILQR_HD double fleet_d2(double ax, double ay, double az, double bx, double by, double bz) {
  const double ex = ax - bx, ey = ay - by, ez = az - bz;
  return fma(ez, ez, fma(ey, ey, ex * ex));
}
// the running minimum over the knots, from (+inf, -1): strict <, so the first knot wins a tie and a NaN never enters
QILQR_HD void fleet_pair_step(double d2, int i, double &best, int &knot) {
  if (d2 < best) {
    best = d2;
    knot = i;
  }
}

// the total order of two candidates (d2 is never a NaN: fleet_pair_step)
QILQR_HD bool fleet_before(double d2a, int rowa, double d2b, int rowb) { return d2a < d2b || (d2a == d2b && rowa < rowb); }

// a sorted list of the K smallest candidates; entry j lies at [j * st] of the three arrays (st = 64: a lane's column of an LDS image;
// st = 1 on the host).  Empty entries are (+inf, FLEET_NO_ROW, -1): behind every candidate.
struct FleetList {
  double *d2;
  int *row, *knot;
  int st, K;
};
QILQR_HD void fleet_list_clear(const FleetList &l) {
  for (int j = 0; j < l.K; ++j) {
    l.d2[j * l.st] = fleet_inf();
    l.row[j * l.st] = FLEET_NO_ROW;
    l.knot[j * l.st] = -1;
  }
}
// offers a candidate: it enters if it lies before the list's last entry (wd2, wrow: the caller's copy of that entry, kept up to date
// here, so that the common refusal touches no memory)
QILQR_HD void fleet_list_offer(const FleetList &l, double &wd2, int &wrow, double d2, int row, int knot) {
  if (!fleet_before(d2, row, wd2, wrow)) return;
  int j = l.K - 1;
  while (j > 0 && fleet_before(d2, row, l.d2[(j - 1) * l.st], l.row[(j - 1) * l.st])) {
    l.d2[j * l.st] = l.d2[(j - 1) * l.st];
    l.row[j * l.st] = l.row[(j - 1) * l.st];
    l.knot[j * l.st] = l.knot[(j - 1) * l.st];
    --j;
  }
  l.d2[j * l.st] = d2;
  l.row[j * l.st] = row;
  l.knot[j * l.st] = knot;
  wd2 = l.d2[(l.K - 1) * l.st];
  wrow = l.row[(l.K - 1) * l.st];
}

// what the summary keeps of all partners of an ego, whatever the yield flag: the closest one under the same order, and how many lie
// closer than `conflict`.  From (+inf, FLEET_NO_ROW, -1, 0); a partner that is nowhere at a finite distance never becomes the closest.
struct FleetBest {
  double d2;
  int row, knot, conflicts;
};
QILQR_HD FleetBest fleet_best_none() { return FleetBest{fleet_inf(), FLEET_NO_ROW, -1, 0}; }
QILQR_HD void fleet_best_pair(FleetBest &s, double d2, int row, int knot, double conflict2) {
  if (knot >= 0 && fleet_before(d2, row, s.d2, s.row)) {
    s.d2 = d2;
    s.row = row;
    s.knot = knot;
  }
  if (d2 < conflict2) s.conflicts += 1;
}
QILQR_HD void fleet_best_merge(FleetBest &s, const FleetBest &o) {
  if (o.knot >= 0 && fleet_before(o.d2, o.row, s.d2, s.row)) {
    s.d2 = o.d2;
    s.row = o.row;
    s.knot = o.knot;
  }
  s.conflicts += o.conflicts;
}

// A vehicle's line p(t) = c + t v through its n knots p_i at t_i = i dt, least squares, per axis and sequentially over the knots:
//   pbar = (sum_i p_i) / n                        tbar = ((n - 1) dt) / 2        Stt = ((dt dt) n (n n - 1)) / 12
//   v = (sum_i fma(t_i - tbar, p_i - pbar, .)) / Stt        c = fma(-tbar, v, pbar)             (n = 1: v = 0, c = p_0)
// and the residual sqrt(max_i |p_i - (fma(t_i, v, c))|^2), the squared norm as fleet_d2 forms it; a line with a word that is not finite
// has the quiet NaN for its residual.  p: word 0 of knot 0's position, the knots `step` words apart.  fit: FLEET_FIT words.
QILQR_HD void fleet_fit_axis(const double *p, long step, int n, double dt, double tbar, double stt, double &c, double &v) {
  double sum = 0.0;
  for (int i = 0; i < n; ++i) sum += p[i * step];
  const double pbar = sum / (double)n;
  double acc = 0.0;
  for (int i = 0; i < n; ++i) acc = fma((double)i * dt - tbar, p[i * step] - pbar, acc);
  v = n > 1 ? acc / stt : 0.0;
  c = fma(-tbar, v, pbar);
}
QILQR_HD void fleet_fit(const double *p, long step, int n, double dt, double *fit) {
  const double tbar = ((double)(n - 1) * dt) * 0.5;
  const double stt = ((dt * dt) * (double)n * ((double)n * (double)n - 1.0)) / 12.0;
  double cx, cy, cz, vx, vy, vz;
  fleet_fit_axis(p, step, n, dt, tbar, stt, cx, vx);
  fleet_fit_axis(p + 1, step, n, dt, tbar, stt, cy, vy);
  fleet_fit_axis(p + 2, step, n, dt, tbar, stt, cz, vz);
  double r2 = 0.0;
  for (int i = 0; i < n; ++i) {
    const double t = (double)i * dt;
    const double d2 = fleet_d2(p[i * step], p[i * step + 1], p[i * step + 2], fma(t, vx, cx), fma(t, vy, cy), fma(t, vz, cz));
    if (!(d2 <= r2) && r2 == r2) r2 = d2;  // (a NaN enters and stays: the fit is then not finite)
  }
  const double res = sqrt(r2);
  fit[0] = cx; fit[1] = cy; fit[2] = cz;
  fit[3] = vx; fit[4] = vy; fit[5] = vz;
  const bool ok = fleet_finite(cx) && fleet_finite(cy) && fleet_finite(cz) && fleet_finite(vx) && fleet_finite(vy) && fleet_finite(vz) && fleet_finite(res);
  fit[6] = ok ? res : __builtin_nan("");  // (the one NaN: the residual is a reported word, and an arithmetic NaN's sign is the machine's)
  fit[7] = ok ? 1.0 : 0.0;
}

// the rule's numbers as the selection reads them
struct FleetSelectRule {
  double radius, weight, range2, conflict2;  // range2, conflict2: fleet_square of the rule's (range = +inf stays +inf)
  unsigned flags;
};

// An ego's outputs from its merged list (entries 0 .. K - 1 under the order), its FleetBest over all partners and the fits of the batch
// (fits[row * FLEET_FIT]).  Any of the four rows may be null.  nbr: K x FLEET_NBR; spheres: K x OB_BWORDS; summary: FLEET_SUMMARY.
// The neighbours are the leading entries with d2 < range2 (an infinite d2 is never below it); each becomes a sphere unless its
// vehicle's fit is not finite, the spheres in the list's order without gaps, zeros behind them.
QILQR_HD void fleet_select_write(const FleetList &l, const FleetBest &best, const double *fits, const FleetSelectRule &r, double *nbr, double *spheres,
                                 int32_t *count, double *summary) {
  int kept = 0;
  double rmax = 0.0;
  bool within = true;
  for (int j = 0; j < l.K; ++j) {
    const double d2 = l.d2[j * l.st];
    const int row = l.row[j * l.st];
    const bool listed = row != FLEET_NO_ROW;
    const double *fit = listed ? fits + (long)row * FLEET_FIT : nullptr;
    if (nbr) {
      nbr[j * FLEET_NBR] = listed ? (double)row : -1.0;
      nbr[j * FLEET_NBR + 1] = sqrt(d2);
      nbr[j * FLEET_NBR + 2] = (double)l.knot[j * l.st];
      nbr[j * FLEET_NBR + 3] = listed ? fit[6] : 0.0;
    }
    within = within && listed && d2 < r.range2 && fleet_finite(d2);
    if (within && fit[7] != 0.0) {
      const double radius = (r.flags & FLEET_COVER) ? r.radius + fit[6] : r.radius;
      if (spheres) {
        double *sp = spheres + kept * OB_BWORDS;
        for (int k = 0; k < 6; ++k) sp[k] = fit[k];
        sp[OB_BRADIUS] = radius;
        sp[OB_BWEIGHT] = r.weight;
      }
      if (radius > rmax) rmax = radius;
      ++kept;
    }
  }
  if (spheres)
    for (int k = kept * OB_BWORDS; k < l.K * OB_BWORDS; ++k) spheres[k] = 0.0;
  if (count) *count = kept;
  if (summary) {
    const bool any = best.knot >= 0;
    summary[0] = any ? sqrt(best.d2) : fleet_inf();
    summary[1] = any ? (double)best.knot : -1.0;
    summary[2] = any ? (double)best.row : -1.0;
    summary[3] = (double)best.conflicts;
    summary[4] = (double)kept;
    summary[5] = rmax;
    summary[6] = summary[7] = 0.0;
  }
}

// ---- qilqr_set_batch_obstacles_device: the rule of a row, and one problem's rows into the tiled table
// a used row is kept unless it has a non-finite word, radius <= 0 or weight < 0 (the refusals of bob_check, as a rule)
QILQR_HD bool bob_row_kept(const double *sp) {
  bool ok = true;
  for (int w = 0; w < OB_BWORDS; ++w) ok = ok && fleet_finite(sp[w]);
  return ok && sp[OB_BRADIUS] > 0.0 && sp[OB_BWEIGHT] >= 0.0;
}
// Problem `row` of the table `tab` (bob_index; K rows): the kept rows among the first clamp(count, 0, K) of `spheres` (K x OB_BWORDS,
// row-major; null: a row of the last tile's padding) in order and without gaps, zeros behind them.  Returns the number kept and adds the
// number dropped to *dropped.
QILQR_HD int bob_set_problem(const double *spheres, int count, int K, double *tab, long row, int *dropped) {
  const int used = !spheres ? 0 : (count < 0 ? 0 : (count > K ? K : count));
  int kept = 0;
  for (int j = 0; j < used; ++j) {
    const double *sp = spheres + j * OB_BWORDS;
    if (!bob_row_kept(sp)) continue;
    for (int w = 0; w < OB_BWORDS; ++w) tab[bob_index(row, K, kept, w)] = sp[w];
    ++kept;
  }
  for (int j = kept; j < K; ++j)
    for (int w = 0; w < OB_BWORDS; ++w) tab[bob_index(row, K, j, w)] = 0.0;
  *dropped += used - kept;
  return kept;
}

// ---- how a call is cut: ego tiles of 64 lanes, and per ego at most FLEET_MAX_CHUNKS chunks of partners of at least FLEET_MIN_CHUNK
constexpr int FLEET_TILE = 64, FLEET_MAX_CHUNKS = 16, FLEET_MIN_CHUNK = 64;
constexpr int FLEET_PT = 16;  // partners a lane holds a running minimum for at once
QILQR_HD int fleet_chunks(int V) {
  const int c = (V + FLEET_MIN_CHUNK - 1) / FLEET_MIN_CHUNK;
  return c > FLEET_MAX_CHUNKS ? FLEET_MAX_CHUNKS : c;
}
QILQR_HD int fleet_chunk_size(int V) { return (V + fleet_chunks(V) - 1) / fleet_chunks(V); }
// a staged row of positions holds V words and FLEET_PT of padding, which a partner tile may read and never uses: the padding is
// deliberately left uninitialised (k_fleet_fit never writes it; what k_fleet_pairs reads of it belongs to partners >= its chunk's end,
// whose running minima are discarded)
QILQR_HD long fleet_row_words(int V) { return (long)((V + FLEET_PT + 1) & ~1); }

}  // namespace qilqr

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
