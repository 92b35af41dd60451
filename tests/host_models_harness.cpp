// host_models_harness.cpp -- CPU test harness (tests only, never part of the product library): the per-problem models extension
// (qilqr_set_batch_models; quadrotorilqr_amd/csrc/batch_models.h, host_model.h) compiled with g++, for tests/test_batch_models_cpu.py.
#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/backward_layout.h"
#include "../quadrotorilqr_amd/csrc/host_model.h"

using namespace qilqr;

extern "C" {

int hm_words() { return PM_WORDS; }
int hm_consts_size() { return (int)sizeof(ModelConsts<double>); }

// the setter's table (make_model_table): -1, or the index of the first bad model
long hm_model_table(const qilqr_model *models, long B, const double *Q, const double *R, double dt, double *tab) {
  return make_model_table(models, B, Q, R, dt, tab);
}

// the handle's own constants (make_model_consts, as qilqr_create builds them): 0, or 1 for a bad inertia
int hm_model_consts(const qilqr_model *m, const double *Q, const double *R, double dt, ModelConsts<double> *out) {
  return make_model_consts(m->mass_kg, m->inertia, m->arm_length_m, m->torque_to_thrust_ratio_m, m->g_mpss, Q, R, dt, out) ? 0 : 1;
}

// Problem b of a batch, as the kernels of the extension see it: the constants through the accessor (problem_model: the shared ones of
// `shared` with row b of `tab`), one step of the device code (discrete_step, or rk4_step with integ = 1) from x = [t(3), q(w,x,y,z),
// v(6)] under u, and the dynamics half of its knot record (linearize_knot, the layout k_linearize writes for diagonal weights) read
// back as the backward kernel reads it: J_x from the record, J_u from the record (the Runge-Kutta extension's dense M) or -- the Euler
// layouts -- rows 0..7 from the shared constant table and rows 8..11 from the problem's record (k_backward_models' operand pointers).
void hm_problem_step(const ModelConsts<double> *shared, const double *tab, long b, int integ, const double *x, const double *u,
                     double *xn, double *Jx, double *Ju) {
  const ModelConsts<double> m = problem_model(*shared, BatchModels{tab}, b);
  double t[3] = {x[0], x[1], x[2]}, q[4] = {x[4], x[5], x[6], x[3]}, v[6];
  for (int i = 0; i < 6; ++i) v[i] = x[7 + i];
  if (integ == 1) {
    double MU[192];
    rk4_step(m, t, q, v, u, MU);
  } else {
    discrete_step(m, t, q, v, u);
  }
  xn[0] = t[0]; xn[1] = t[1]; xn[2] = t[2];
  xn[3] = q[3]; xn[4] = q[0]; xn[5] = q[1]; xn[6] = q[2];
  for (int i = 0; i < 6; ++i) xn[7 + i] = v[i];

  const RecLayout L = make_layout(true, true, integ == 1);
  double pt[18] = {0.0}, pd[18] = {0.0}, rec[LIN_MAX_STRIDE] = {0.0};
  for (int i = 0; i < 13; ++i) pt[1 + i] = x[i];
  for (int a = 0; a < 4; ++a) pt[14 + a] = u[a];
  pd[4] = 1.0;
  linearize_knot(m, L, pt, pd, rec);
  double ctab[CTAB_SIZE];
  build_ctab(shared->Bu, shared->Q, ctab);
  const double *pm = tab + b * PM_WORDS;
  for (int r = 0; r < 12; ++r)
    for (int col = 0; col < 16; ++col) {
      const int src = m_source_tab(L, r, col);
      double v;
      if (src >= 0) v = rec[src];
      else if (col >= 12 && r >= PM_BU_ROW0) v = pm[PM_BU + (r - PM_BU_ROW0) * 4 + (col - 12)];
      else v = ctab[-1 - src];
      if (col < 12) Jx[r * 12 + col] = v;
      else Ju[r * 4 + (col - 12)] = v;
    }
}

}  // extern "C"
