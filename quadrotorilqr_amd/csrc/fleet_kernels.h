// fleet_kernels.h -- fleet deconfliction on the device: who is near whom over the horizon, as spheres.
//   k_fleet_fit      one lane per vehicle: its constant-velocity line (fleet_fit) into fit[B][8], and its positions staged into
//                    pos[fleet][knot][axis][fleet_row_words(V)], so that the 64 egos of a tile load a word of a knot as one 512-byte read
//                    and the partners of a tile lie side by side
//   k_fleet_pairs    THE HOT PATH.  One wavefront per (ego tile, partner chunk, fleet); a lane is an ego.  FLEET_PT partners at a
//                    time: per knot the ego's three words are loaded once and used against the FLEET_PT partners, whose words are
//                    uniform across the lanes (the addresses are made of the block's index and loop counters only: scalar loads).
//                    Per pair a running minimum and its knot in registers (fleet_pair_step); behind the knot loop a pair is offered
//                    to the lane's list of its K best, a column of an LDS image, whose last entry the lane keeps in registers: the
//                    divergent insertion runs only for a pair that beats it.  Writes per (chunk, ego) the list and the FleetBest.
//                    No position is kept in LDS, so no horizon is too long for it.
//   k_fleet_select   one lane per ego: merges the chunks' lists under the same order (again through an LDS column), merges the
//                    FleetBest, and writes the outputs (fleet_select_write).
//   k_bob_set        qilqr_set_batch_obstacles_device: one lane per problem of the tiled table, the padding rows of the last tile
//                    included; a sequential loop over the K rows (bob_set_problem).
// (d2, partner row) is a total order, so an ego's list does not depend on the chunks: tests/test_fleet_cpu.py runs the same routines on the
// host with chunks of 1, 7, 64 and V partners.  No kernel uses scratch memory; the unit's register table is in DESIGN.md.
#pragma once

#include <hip/hip_runtime.h>

#include "fleet_math.h"

namespace qilqr {

struct FleetFitArgs {
  const double *plan;  // [B][n][18]
  double *pos, *fit;
  int B, n, V;
  long row_words;      // fleet_row_words(V)
  double dt;
};
__global__ __launch_bounds__(FLEET_TILE) void k_fleet_fit(FleetFitArgs a) {
  const long b = (long)blockIdx.x * FLEET_TILE + threadIdx.x;
  if (b >= a.B) return;
  const double *p = a.plan + b * a.n * 18 + 1;
  fleet_fit(p, 18, a.n, a.dt, a.fit + b * FLEET_FIT);
  double *out = a.pos + (b / a.V) * a.n * 3 * a.row_words + b % a.V;
  for (int i = 0; i < a.n; ++i)
    for (int k = 0; k < 3; ++k) out[(i * 3l + k) * a.row_words] = p[i * 18l + k];
}

struct FleetPairsArgs {
  double *pd2;   // [C][K][B]
  int2 *prk;     // [C][K][B]: (row, knot)
  double *sd2;   // [C][B]
  int2 *srk;     // [C][B]
  int *sconf;    // [C][B]
  int B, n, V, K, C, P, tiles;  // C chunks of P partners; ego tiles per fleet
  long row_words;
  double conflict2;
  unsigned flags;
};
__global__ __launch_bounds__(FLEET_TILE) void k_fleet_pairs(const double *__restrict__ pos, FleetPairsArgs a) {
  __shared__ double l_d2[FLEET_MAX_NEIGHBOURS * FLEET_TILE];
  __shared__ int l_row[FLEET_MAX_NEIGHBOURS * FLEET_TILE], l_knot[FLEET_MAX_NEIGHBOURS * FLEET_TILE];
  const int lane = threadIdx.x;
  const int tile = blockIdx.x % a.tiles, c = blockIdx.x / a.tiles % a.C, g = blockIdx.x / a.tiles / a.C;
  const int ev = tile * FLEET_TILE + lane;       // the ego within its fleet
  const bool live = ev < a.V;
  const int el = live ? ev : a.V - 1;            // (the lanes behind the fleet's end load its last vehicle and write nothing)
  const FleetList list{l_d2 + lane, l_row + lane, l_knot + lane, FLEET_TILE, a.K};
  fleet_list_clear(list);
  double wd2 = fleet_inf();
  int wrow = FLEET_NO_ROW;
  FleetBest best = fleet_best_none();
  const int pbeg = c * a.P, pend = pbeg + a.P < a.V ? pbeg + a.P : a.V;
  const double *fp = pos + (long)g * a.n * 3 * a.row_words;
  for (int p0 = pbeg; p0 < pend; p0 += FLEET_PT) {
    double m[FLEET_PT];
    int mk[FLEET_PT];
#pragma unroll
    for (int j = 0; j < FLEET_PT; ++j) {
      m[j] = fleet_inf();
      mk[j] = -1;
    }
    for (int i = 0; i < a.n; ++i) {
      const double *rx = fp + i * 3l * a.row_words, *ry = rx + a.row_words, *rz = ry + a.row_words;
      const double ax = rx[el], ay = ry[el], az = rz[el];
#pragma unroll
      for (int j = 0; j < FLEET_PT; ++j) fleet_pair_step(fleet_d2(ax, ay, az, rx[p0 + j], ry[p0 + j], rz[p0 + j]), i, m[j], mk[j]);  // (p0 + j < V + FLEET_PT: the row's padding)
    }
#pragma unroll
    for (int j = 0; j < FLEET_PT; ++j) {
      const int pv = p0 + j;
      if (!live || pv >= pend || pv == ev) continue;
      const int row = g * a.V + pv;
      fleet_best_pair(best, m[j], row, mk[j], a.conflict2);
      if (!(a.flags & FLEET_YIELD_TO_LOWER) || pv < ev) fleet_list_offer(list, wd2, wrow, m[j], row, mk[j]);
    }
  }
  if (!live) return;
  const long ego = (long)g * a.V + ev;
  for (int k = 0; k < a.K; ++k) {
    const long at = ((long)c * a.K + k) * a.B + ego;
    a.pd2[at] = list.d2[k * FLEET_TILE];
    a.prk[at] = make_int2(list.row[k * FLEET_TILE], list.knot[k * FLEET_TILE]);
  }
  a.sd2[(long)c * a.B + ego] = best.d2;
  a.srk[(long)c * a.B + ego] = make_int2(best.row, best.knot);
  a.sconf[(long)c * a.B + ego] = best.conflicts;
}

struct FleetSelectArgs {
  const double *pd2;
  const int2 *prk;
  const double *sd2;
  const int2 *srk;
  const int *sconf;
  const double *fit;
  int B, K, C;
  FleetSelectRule rule;
  double *summary, *nbr, *spheres;
  int32_t *counts;
};
__global__ __launch_bounds__(FLEET_TILE) void k_fleet_select(FleetSelectArgs a) {
  __shared__ double l_d2[FLEET_MAX_NEIGHBOURS * FLEET_TILE];
  __shared__ int l_row[FLEET_MAX_NEIGHBOURS * FLEET_TILE], l_knot[FLEET_MAX_NEIGHBOURS * FLEET_TILE];
  const int lane = threadIdx.x;
  const long b = (long)blockIdx.x * FLEET_TILE + lane;
  if (b >= a.B) return;
  const FleetList list{l_d2 + lane, l_row + lane, l_knot + lane, FLEET_TILE, a.K};
  fleet_list_clear(list);
  double wd2 = fleet_inf();
  int wrow = FLEET_NO_ROW;
  FleetBest best = fleet_best_none();
  for (int c = 0; c < a.C; ++c) {
    for (int k = 0; k < a.K; ++k) {
      const long at = ((long)c * a.K + k) * a.B + b;
      const int2 rk = a.prk[at];
      if (rk.x == FLEET_NO_ROW) break;  // (a chunk's list is sorted: nothing behind an empty entry)
      fleet_list_offer(list, wd2, wrow, a.pd2[at], rk.x, rk.y);
    }
    const int2 rk = a.srk[(long)c * a.B + b];
    fleet_best_merge(best, FleetBest{a.sd2[(long)c * a.B + b], rk.x, rk.y, a.sconf[(long)c * a.B + b]});
  }
  fleet_select_write(list, best, a.fit, a.rule, a.nbr ? a.nbr + b * a.K * FLEET_NBR : nullptr, a.spheres ? a.spheres + b * a.K * OB_BWORDS : nullptr,
                     a.counts ? a.counts + b : nullptr, a.summary ? a.summary + b * FLEET_SUMMARY : nullptr);
}

struct BobSetArgs {
  const double *spheres;
  const int32_t *counts;
  double *tab;
  int32_t *tab_counts, *dropped;
  int B, K;
};
__global__ __launch_bounds__(OB_TILE) void k_bob_set(BobSetArgs a) {
  const long row = (long)blockIdx.x * OB_TILE + threadIdx.x;  // (the grid is the table's tiles: the last one's padding rows are zeroed)
  int dropped = 0;
  if (row < a.B) a.tab_counts[row] = bob_set_problem(a.spheres + row * a.K * OB_BWORDS, a.counts ? a.counts[row] : a.K, a.K, a.tab, row, &dropped);
  else bob_set_problem(nullptr, 0, a.K, a.tab, row, &dropped);
  if (a.dropped && dropped) atomicAdd(a.dropped, dropped);
}

}  // namespace qilqr
