// host_shift_harness.cpp -- CPU test harness (tests only, never part of the product library): the device routines of the receding-horizon
// shift (quadrotorilqr_amd/csrc/shift_kernels.h: shift_copy_pair, shift_tail_problem) and the index checks of the horizon start
// (horizon.h) compiled with g++, for tests/test_shift_cpu.py.
#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/horizon.h"
#include "../quadrotorilqr_amd/csrc/host_model.h"
#include "../quadrotorilqr_amd/csrc/shift_kernels.h"

using namespace qilqr;

extern "C" {

int hsf_words() { return PM_WORDS; }
int hsf_consts_size() { return (int)sizeof(ModelConsts<double>); }

// the handle's constants (make_model_consts) and the per-problem records (make_model_table), as the library builds them
int hsf_model_consts(const qilqr_model *m, const double *Q, const double *R, double dt, ModelConsts<double> *out) {
  return make_model_consts(m->mass_kg, m->inertia, m->arm_length_m, m->torque_to_thrust_ratio_m, m->g_mpss, Q, R, dt, out) ? 0 : 1;
}
long hsf_model_table(const qilqr_model *models, long B, const double *Q, const double *R, double dt, double *tab) {
  return make_model_table(models, B, Q, R, dt, tab);
}

// One launch of k_shift as the grid runs it: every copy pair through shift_copy_pair, every problem's lane through shift_tail_problem
// (integ, limits lo / hi or null, model records tab or null).  `writes` ([B][n][18] ints, zeroed by the caller) counts the routine calls
// that stored into each output word: before every call the whole output is set to a NaN payload no routine produces, and what the call
// leaves different is what it wrote -- so the test sees that each word has exactly one writer, wherever a routine writes.
extern "C++" {
namespace {
const unsigned long long SENTINEL = 0x7ff8dead0000beefull;
template <typename F>
void counted(double *out, double *saved, long words, int *writes, F call) {
  double mark;
  __builtin_memcpy(&mark, &SENTINEL, sizeof mark);
  for (long w = 0; w < words; ++w) {
    saved[w] = out[w];
    out[w] = mark;
  }
  call();
  for (long w = 0; w < words; ++w) {
    if (__builtin_memcmp(out + w, &SENTINEL, sizeof(double)) != 0) ++writes[w];
    else out[w] = saved[w];
  }
}
}  // namespace
}  // extern "C++"
int hsf_shift(const ModelConsts<double> *c, const double *tab, const double *in, const double *x0, double *out, int B, int n, int steps,
              int tail, int integ, const double *lo, const double *hi, int *writes) {
  if (tail != SHIFT_TAIL_HOLD && tail != SHIFT_TAIL_HOVER) return 1;
  ShiftArgs a{in, x0, out, B, n, steps, tail, (steps > 0 || x0) ? (B + SHIFT_BLOCK - 1) / SHIFT_BLOCK : 0};
  const long words = (long)B * n * 18;
  double *saved = new double[words];
  const long pairs = shift_copy_pairs(a);
  for (long g = 0; g < pairs; ++g) counted(out, saved, words, writes, [&] { shift_copy_pair(a, g); });
  for (int b = 0; b < B && a.tail_blocks > 0; ++b) {
    const ModelConsts<double> m = tab ? problem_model(*c, BatchModels{tab}, (long)b) : *c;
    const double *pi = in + (long)b * n * 18, *px = x0 ? x0 + (long)b * SHIFT_STATE : nullptr;
    double *po = out + (long)b * n * 18;
    counted(out, saved, words, writes, [&] {
      if (integ == 1 && lo) shift_tail_problem<1, true>(m, pi, px, po, n, steps, tail, lo, hi);
      else if (integ == 1) shift_tail_problem<1, false>(m, pi, px, po, n, steps, tail);
      else if (lo) shift_tail_problem<0, true>(m, pi, px, po, n, steps, tail, lo, hi);
      else shift_tail_problem<0, false>(m, pi, px, po, n, steps, tail);
    });
  }
  delete[] saved;
  return 0;
}

// horizon.h: the setter's check and a call's (-1: a refusal without a reason, or a reason without a refusal)
int hsf_start_check(long k0, long n_desired, long n_sched) {
  const char *why = nullptr;
  const int rc = horizon_start_check(k0, n_desired, n_sched, &why);
  return (rc != HZ_OK) == (why != nullptr) ? rc : -1;
}
int hsf_window_check(long n, long k0, long n_desired, long n_sched, int shared_desired, int evaluates_cost) {
  const char *why = nullptr;
  const int rc = horizon_window_check(n, k0, n_desired, n_sched, shared_desired != 0, evaluates_cost != 0, &why);
  return (rc != HZ_OK) == (why != nullptr) ? rc : -1;
}
int hsf_schedule_check(long k0, long n_knots) {
  const char *why = nullptr;
  const int rc = horizon_schedule_check(k0, n_knots, &why);
  return (rc != HZ_OK) == (why != nullptr) ? rc : -1;
}

}  // extern "C"
