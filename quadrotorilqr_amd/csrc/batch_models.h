// batch_models.h -- per-problem quadrotor models of a batch (qilqr_set_batch_models, an extension the reference does not have): problem b
// of the batch is solved with its own mass, g, inertia and moment arms; dt, Q, R, the desired trajectory and the options stay the handle's.
//
// One compact record per problem, PM_WORDS doubles, built on the host from make_model_consts (host_model.h: make_model_table, so every
// field has the bits a handle created with that model would have) and uploaded once per setter call.  The kernels of the extension take
// the table as a trailing argument of their own (BatchModels) and index it by the problem's row, st.row0 + slot (the compaction, the only
// thing that moves a trajectory to another slot, is off while models are set).  ModelConsts (the shared constants, passed by value) and
// SolveParams do not change: no pre-existing kernel sees the table.  Compiles under g++ (QILQR_HD, se3_math.h).
#pragma once

#include <type_traits>

#include "se3_math.h"

namespace qilqr {

// record layout: mass, g, inertia (3 x 3), inertia^-1 (3 x 3), moment arms (3 x 4), rows 8..11 of the constant J_u (4 x 4: dt / m and
// dt I^-1 moment_arms; rows 0..7 are zero for every model)
constexpr int PM_MASS = 0, PM_G = 1, PM_INERTIA = 2, PM_INERTIA_INV = 11, PM_ARMS = 20, PM_BU = 32, PM_WORDS = 48;
constexpr int PM_BU_ROW0 = 8;  // the first row of J_u a record holds

// the table as a kernel argument: [rows][PM_WORDS], fp64
struct BatchModels {
  const double *tab;
};

// ModelConsts -> record (host: make_model_table)
QILQR_HD void pack_problem_model(const ModelConsts<double> &c, double *rec) {
  rec[PM_MASS] = c.mass;
  rec[PM_G] = c.g;
  for (int i = 0; i < 9; ++i) rec[PM_INERTIA + i] = c.inertia[i];
  for (int i = 0; i < 9; ++i) rec[PM_INERTIA_INV + i] = c.inertia_inv[i];
  for (int i = 0; i < 12; ++i) rec[PM_ARMS + i] = c.arms[i];
  for (int i = 0; i < 16; ++i) rec[PM_BU + i] = c.Bu[PM_BU_ROW0 * 4 + i];
}

// The accessor: the constants of the problem whose record is `rec` -- the shared ones (dt, Q, R, the zero rows of J_u) with the record's
// model fields.  What the dynamics code (discrete_step, rk4_step, linearize_dynamics[_rk4], rollout_problem) reads of a ModelConsts.
template <typename T>
QILQR_HD ModelConsts<T> problem_model(const ModelConsts<T> &shared, const double *rec) {
  ModelConsts<T> m = shared;
  m.mass = (T)rec[PM_MASS];
  m.g = (T)rec[PM_G];
#pragma unroll
  for (int i = 0; i < 9; ++i) m.inertia[i] = (T)rec[PM_INERTIA + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) m.inertia_inv[i] = (T)rec[PM_INERTIA_INV + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) m.arms[i] = (T)rec[PM_ARMS + i];
#pragma unroll
  for (int i = 0; i < 16; ++i) m.Bu[PM_BU_ROW0 * 4 + i] = (T)rec[PM_BU + i];
  return m;
}
// ... of row `row` of a table
template <typename T>
QILQR_HD ModelConsts<T> problem_model(const ModelConsts<T> &shared, const BatchModels &bm, long row) {
  return problem_model(shared, bm.tab + row * PM_WORDS);
}

// The trailing arguments of a kernel of the extensions (ControlLimits, BatchModels, in any combination): is one of type T there, and
// which is it.
template <typename T, typename... P>
constexpr bool pack_has = (std::is_same<T, P>::value || ...);
template <typename T, typename P0, typename... P>
QILQR_HD const T &pack_get(const P0 &p0, const P &...p) {
  if constexpr (std::is_same<T, P0>::value) return p0;
  else return pack_get<T>(p...);
}

}  // namespace qilqr
