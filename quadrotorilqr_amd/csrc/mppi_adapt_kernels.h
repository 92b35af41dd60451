// mppi_adapt_kernels.h -- the sampling planner's spread per knot and rotor, adapted on the device:
//   k_mppi_flight_spread   k_mppi_flight (mppi_kernels.h) with the perturbation's deviation read per plan, knot and rotor from
//                          spread[B][n][4] instead of the rule's sigma
//   k_mppi_adapt           k_mppi_update with the weighted SECOND moment of the perturbations beside the first: out_plan as the update
//                          makes it, and out_spread[B][n][4], the spread blended towards the weighted deviation
// and mppi.hip's nominal flight behind the second, as behind the update.  The first is mppi_flight_block (mppi_kernels.h) over an LDS
// image and a fetch with the deviations; the second repeats k_mppi_update's head statement for statement and has its own knot loop.
//
// THE PERTURBATION of sample j at knot i, rotor a:  eps_i[a] = spread[b, i, a] * z_i[a], a rounded product, where z is mppi_eps_row's
// recursion with the coefficients of sigma = {1, 1, 1, 1} (mppi_unit_coeffs): z_0 = xi_0, z_i = fma(rho, z_{i-1}, kappa1 xi_i).  The
// nominal sample has eps = 0.  With tau_s = 0 and spread = sigma at every knot eps has the bits of mppi_eps_row's with that sigma.
//
// THE ADAPTATION of plan b: keys, J_min, weights, eta, q and every fold order are k_mppi_update's (the same routines).  Per knot and rotor
//     per sample   t = w_j eps,  m1 += t,  t2 = t eps,  m2 += t2                                     (mppi_fold_moments)
//     du = m1 / eta,  e2 = m2 / eta,  dd = du du,  var = e2 - dd,  not > 0: 0                        (mppi_weighted_var)
//     old2 = s_old s_old,  v = one_minus_rate old2 + rate var,  s_new = clamp(sqrt(v), floor, cap)   (mppi_blend_spread)
// and the new control is mppi_new_control of m1.  Without a finite key the spread is the input's, bit for bit, as the controls are.
#pragma once

#include "mppi_kernels.h"

namespace qilqr {

constexpr int MPPI_SPREAD_PAIRS = 2;  // sixteen-byte pairs of a knot's four deviations

// the unit recursion's coefficients: rho of tau_s, sigma = 1, kappa = sqrt((1 - rho)(1 + rho))
inline void mppi_unit_coeffs(double tau_s, double dt, MppiCoeffs &m) {
  const double one[4] = {1.0, 1.0, 1.0, 1.0};
  mppi_coeffs(one, tau_s, dt, m);
}

// what the host makes of a qilqr_mppi_adapt_rule
struct MppiAdaptCoeffs {
  double floor[4], cap[4], rate, one_minus_rate;
};
inline void mppi_adapt_coeffs(const double floor[4], const double cap[4], double rate, MppiAdaptCoeffs &k) {
  for (int a = 0; a < 4; ++a) {
    k.floor[a] = floor[a];
    k.cap[a] = cap[a];
  }
  k.rate = rate;
  k.one_minus_rate = 1.0 - rate;
}

// (one rounding per operation written, as the folds of mppi_kernels.h)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// eps = spread z, rounded before anything is added to it
QILQR_HD void mppi_spread_eps(const double spread[4], const double z[4], bool nominal, double eps[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) eps[a] = nominal ? 0.0 : spread[a] * z[a];
}
// one sample's terms of the two moments, in the order of mppi_fold_term
QILQR_HD void mppi_fold_moments(double w, const double eps[4], double m1[4], double m2[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const double t = w * eps[a];
    m1[a] += t;
    const double t2 = t * eps[a];
    m2[a] += t2;
  }
}
// the weighted variance of one knot and rotor
QILQR_HD double mppi_weighted_var(double m1, double m2, double eta) {
  const double du = m1 / eta;
  const double e2 = m2 / eta;
  const double dd = du * du;
  const double var = e2 - dd;
  return var > 0.0 ? var : 0.0;
}
// the new deviation of one knot and rotor
QILQR_HD double mppi_blend_spread(double s_old, double var, bool any, double one_minus_rate, double rate, double floor, double cap) {
  if (!any) return s_old;
  const double old2 = s_old * s_old;
  const double keep = one_minus_rate * old2;
  const double take = rate * var;
  const double v = keep + take;
  const double s = sqrt(v);
  return s < floor ? floor : (s > cap ? cap : s);
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

// MppiFlatFetch with plan b's deviations: spread + 4 i are knot i's
struct MppiFlatSpreadFetch : MppiFlatFetch {
  const double *spread;
  QILQR_HD void eps(int i, const double z[4], bool nominal, double e[4]) const { mppi_spread_eps(spread + 4 * (long)i, z, nominal, e); }
};
template <>
struct MppiFetchSpreads<MppiFlatSpreadFetch> {
  static constexpr bool value = true;
};

#if defined(__HIPCC__)
struct MppiFlightSpreadArgs {
  MppiFlightArgs f;      // (f.m: the unit coefficients)
  const double *spread;  // [B][n][4]
};

// MppiImage and the knot's four deviations, two more pairs per half: loaded two knots ahead by lanes 18 and 19 into a register, written
// one knot ahead, read by every lane at one address.  9 600 bytes a block.
struct MppiSpreadImage {
  MppiImage base;
  cl_dv2 spread[2][MPPI_SPREAD_PAIRS];
};

// MppiSharedFetch's scheme with the deviations beside the knot: the barrier of knot i is the base's, and the half that is written behind
// it is the one the lanes read before it
struct MppiSharedSpreadFetch {
  MppiSharedFetch base;
  const cl_dv2 *spread;  // the plan's first knot
  MppiSpreadImage *img;
  cl_dv2 next;
  __device__ bool mine() const { return base.lane >= MPPI_KNOT_PAIRS && base.lane < MPPI_KNOT_PAIRS + MPPI_SPREAD_PAIRS; }
  __device__ cl_dv2 load(int i) const { return spread[(long)i * MPPI_SPREAD_PAIRS + (base.lane - MPPI_KNOT_PAIRS)]; }
  __device__ void prime(const double *sp, int n_shared, const double *own, int K, long b, int n_own) {
    if (mine()) {
      img->spread[0][base.lane - MPPI_KNOT_PAIRS] = load(0);
      if (1 <= base.i1) next = load(1);
    }
    base.prime(sp, n_shared, own, K, b, n_own);
  }
  __device__ void operator()(int i, double pt[18]) {
    base(i, pt);
    if (mine()) {
      if (i + 1 <= base.i1) img->spread[(i + 1) & 1][base.lane - MPPI_KNOT_PAIRS] = next;
      if (i + 2 <= base.i1) next = load(i + 2);
    }
  }
  __device__ ClKnotScore score(int i) const { return base.score(i); }
  __device__ void eps(int i, const double z[4], bool nominal, double e[4]) const {
    const cl_dv2 s01 = img->spread[i & 1][0], s23 = img->spread[i & 1][1];
    const double s[4] = {s01[0], s01[1], s23[0], s23[1]};
    mppi_spread_eps(s, z, nominal, e);
  }
};
template <>
struct MppiFetchSpreads<MppiSharedSpreadFetch> {
  static constexpr bool value = true;
};

// k_mppi_flight's block (mppi_flight_block) over the base of this kernel's image, its fetch wrapped in MppiSharedSpreadFetch with plan b's
// deviations; no trajectory store.
template <int INTEG, typename... Lim>
__global__ __launch_bounds__(CL_BLOCK) void k_mppi_flight_spread(ModelConsts<double> c, MppiFlightSpreadArgs as, Lim... lim) {
  __shared__ MppiSpreadImage image;
  mppi_flight_block<INTEG, false>(c, as.f, image.base, [&](const MppiSharedFetch &base, int b) {
    return MppiSharedSpreadFetch{base, reinterpret_cast<const cl_dv2 *>(as.spread + 4 * (long)b * as.f.n), &image, cl_dv2{0.0, 0.0}};
  }, lim...);
}

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// a word that every lane of the wavefront holds, kept in scalar registers (the 1024-lane block has 128 vector registers a lane)
__device__ __forceinline__ double mppi_wave_uniform(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}

// Lane l's copy of lane (l ^ OFF)'s word.  1, 2 and 8 stay inside a row of sixteen lanes and are data-parallel moves (quad_perm, a
// rotation by 8): no LDS cycle; 4, 16 and 32 are __shfl_xor, as every step of k_mppi_update is.  The same word arrives either way, so
// the butterfly's sums have the update's bits -- and eight accumulators cost the LDS what the update's four do.
template <int OFF>
__device__ __forceinline__ double mppi_from_xor(double x) {
  if constexpr (OFF == 1 || OFF == 2 || OFF == 8) {
    constexpr int CTRL = OFF == 1 ? 0xB1 : (OFF == 2 ? 0x4E : 0x128);
    const long long v = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(v >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
  } else {
    return __shfl_xor(x, OFF);
  }
}
template <int OFF>
__device__ __forceinline__ void mppi_butterfly_step(double acc[4], double acc2[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    acc[r] += mppi_from_xor<OFF>(acc[r]);
    acc2[r] += mppi_from_xor<OFF>(acc2[r]);
  }
}

struct MppiAdaptArgs {
  MppiUpdateArgs u;      // (u.m: the unit coefficients)
  const double *spread;  // [B][n][4]
  double *out_spread;    // [B][n][4], or null: the mean only
  MppiAdaptCoeffs k;
};

// k_mppi_update's form and grid, statement for statement up to the weighted perturbations: one block of THREADS = mppi_update_lanes(S)
// lanes per plan.  Then four more accumulators a lane, part2 beside part, the knot's deviations read by every lane at one address (from LDS,
// a chunk's rows at a time), and out_spread written where the controls are.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_mppi_adapt(const MppiAdaptArgs aa) {
  constexpr int WAVES = THREADS / 64;
  const MppiUpdateArgs &a = aa.u;
  __shared__ double weights[THREADS == MPPI_UPDATE_MAX_THREADS ? MPPI_MAX_SAMPLES : THREADS];  // (below the cap S <= THREADS)
  __shared__ double part[MPPI_CHUNK][WAVES][4], part2[MPPI_CHUNK][WAVES][4];
  __shared__ double wmin_key[WAVES], wsum[2][WAVES];
  __shared__ int wmin_j[WAVES], wmin_n[WAVES];
  // a rotor's limits, floor and cap, read where a word is written: held in registers through the knots they would not fit beside the
  // recursion states of four samples (the 1024-lane block has 128 vector registers a lane)
  __shared__ double rotor[4][4];
  // the deviations of a chunk's knots, fetched while the chunk before is combined: a knot's row is then an LDS broadcast and the knot
  // loop holds no global load (measured at 64 x 1024 x 100: the same time as a load per knot -- DESIGN.md section 8p)
  __shared__ __attribute__((aligned(16))) double rows[MPPI_CHUNK * 4];
  const int t = (int)threadIdx.x, wave = t >> 6, b = (int)blockIdx.x, S = a.S, n = a.n;
  if (t == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      rotor[0][r] = a.lim_lo[r];
      rotor[1][r] = a.lim_hi[r];
      rotor[2][r] = aa.k.floor[r];
      rotor[3][r] = aa.k.cap[r];
    }
  }  // (read behind the barriers below)
  const double *plan = a.plan + (long)b * n * 18, *mine = a.score + 4 * (long)b * S, *spread = aa.spread + 4 * (long)b * n;
  double *out = a.out_plan + (long)b * n * 18, *out_spread = aa.out_spread ? aa.out_spread + 4 * (long)b * n : nullptr;
  if (t < 4 * (n < MPPI_CHUNK ? n : MPPI_CHUNK)) rows[t] = spread[t];
  // time and states: pairs 0 .. 6 of every knot, word for word (pairs 7 and 8, the controls, are written below)
  for (long p = t; p < 7l * n; p += THREADS) {
    const long i = p / 7, e = p - 7 * i;
    reinterpret_cast<cl_dv2 *>(out)[i * 9 + e] = reinterpret_cast<const cl_dv2 *>(plan)[i * 9 + e];
  }
  // J_min, its sample and the count of finite keys
  MppiMin f = mppi_lane_min(mine, S, t, THREADS, a.collision_cost);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) f = mppi_min_combine(f, mppi_min_from(f, off));
  if ((t & 63) == 0) {
    wmin_key[wave] = f.key;
    wmin_j[wave] = f.j;
    wmin_n[wave] = f.n_finite;
  }
  __syncthreads();
  f = MppiMin{wmin_key[0], wmin_j[0], wmin_n[0]};
  for (int w = 1; w < WAVES; ++w) f = mppi_min_combine(f, MppiMin{wmin_key[w], wmin_j[w], wmin_n[w]});
  const bool any = f.j >= 0;
  // the weights, then eta and q
  for (int j = t; j < S; j += THREADS) weights[j] = any ? mppi_weight(mppi_key(mine + 4 * (long)j, a.collision_cost), f.key, a.lambda) : 0.0;
  double eta, q;
  mppi_lane_weights(weights, S, t, THREADS, eta, q);  // (a lane reads back what it wrote: no barrier)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    eta += __shfl_xor(eta, off);
    q += __shfl_xor(q, off);
  }
  if ((t & 63) == 0) {
    wsum[0][wave] = eta;
    wsum[1][wave] = q;
  }
  __syncthreads();
  eta = mppi_waves_in_order(wsum[0], WAVES, 1);
  q = mppi_waves_in_order(wsum[1], WAVES, 1);
  if (t == 0) {
    double w4[4];
    mppi_info_words(f, eta, q, w4);
    cl_store_pair(a.info + (long)b * MPPI_INFO, w4[0], w4[1]);
    cl_store_pair(a.info + (long)b * MPPI_INFO + 2, w4[2], w4[3]);
  }
  // the two weighted moments of the perturbations, MPPI_CHUNK knots between two combinations of the wavefronts
  double g[MPPI_PER_LANE][4];
#pragma unroll
  for (int k = 0; k < MPPI_PER_LANE; ++k) g[k][0] = g[k][1] = g[k][2] = g[k][3] = 0.0;
  const uint32_t pl = a.b0 + (uint32_t)b;
  for (int c0 = 0; c0 < n; c0 += MPPI_CHUNK) {
    const int now = n - c0 < MPPI_CHUNK ? n - c0 : MPPI_CHUNK;
    for (int ii = 0; ii < now; ++ii) {
      const cl_dv2 s01 = reinterpret_cast<const cl_dv2 *>(rows)[2 * ii], s23 = reinterpret_cast<const cl_dv2 *>(rows)[2 * ii + 1];
      double sp[4] = {s01[0], s01[1], s23[0], s23[1]};
#pragma unroll
      for (int r = 0; r < 4; ++r) sp[r] = mppi_wave_uniform(sp[r]);
      double acc[4] = {0.0, 0.0, 0.0, 0.0}, acc2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < MPPI_PER_LANE; ++k) {
        const int j = t + k * THREADS;
        if (j < S) {
          const bool nominal = mppi_is_nominal(a.flags, j);
          mppi_eps_row(a.m, a.seed, pl, (uint32_t)j, (uint32_t)(c0 + ii), nominal, g[k]);
          double e[4];
          mppi_spread_eps(sp, g[k], nominal, e);
          mppi_fold_moments(weights[j], e, acc, acc2);
        }
      }
      mppi_butterfly_step<32>(acc, acc2);
      mppi_butterfly_step<16>(acc, acc2);
      mppi_butterfly_step<8>(acc, acc2);
      mppi_butterfly_step<4>(acc, acc2);
      mppi_butterfly_step<2>(acc, acc2);
      mppi_butterfly_step<1>(acc, acc2);
      if ((t & 63) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          part[ii][wave][r] = acc[r];
          part2[ii][wave][r] = acc2[r];
        }
      }
    }
    __syncthreads();
    if (t < 4 * now) {
      const int ii = t >> 2, r = t & 3;
      const double d = mppi_waves_in_order(&part[ii][0][r], WAVES, 4);
      const unsigned w = (unsigned)(c0 + ii) * 18u + 14u + (unsigned)r;  // (offsets inside the plan's own rows, which n bounds)
      const double eta_here = mppi_waves_in_order(wsum[0], WAVES, 1);     // (eta's bits, read again: not carried through the knots)
      const double lo = rotor[0][r], hi = rotor[1][r], floor = rotor[2][r], cap = rotor[3][r];
      out[w] = mppi_new_control(plan[w], d, eta_here, any, a.limited != 0, lo, hi);
      if (out_spread) {
        const unsigned ws = 4u * (unsigned)c0 + (unsigned)t;  // (= 4 (c0 + ii) + r)
        const double d2 = mppi_waves_in_order(&part2[ii][0][r], WAVES, 4);  // (behind the control's store: sixteen wavefronts' words are a lane's registers)
        const double var = any ? mppi_weighted_var(d, d2, eta_here) : 0.0;
        out_spread[ws] = mppi_blend_spread(spread[ws], var, any, aa.k.one_minus_rate, aa.k.rate, floor, cap);
      }
    }
    {  // the next chunk's rows (every lane has read this chunk's before the barrier above)
      const int left = n - (c0 + MPPI_CHUNK), next = left < MPPI_CHUNK ? left : MPPI_CHUNK;
      if (t < 4 * next) rows[t] = spread[4 * (c0 + MPPI_CHUNK) + t];
    }
    __syncthreads();
  }
}
#endif

}  // namespace qilqr

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
