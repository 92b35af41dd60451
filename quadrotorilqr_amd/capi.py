"""ctypes binding of libquadrotor_ilqr.so (include/quadrotor_ilqr.h) and the host-side mirror
of the reference's ILQR<QuadrotorModel> interface (src/ilqr.hh:25-206): same method names,
argument meaning and error behaviour, batched.

There is no CPU fallback: if the HIP library is missing or no GPU is present every compute
entry point raises.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (QILQR_LIB: another build of the same library, for A/B measurements -- profiles/microbench)
LIB_PATH = os.environ.get("QILQR_LIB") or os.path.join(_HERE, "lib", "libquadrotor_ilqr.so")

KNOT = 18
GAIN = 52

OK = 0
ERR_BAD_INERTIA = 1
ERR_LENGTH_MISMATCH = 2
ERR_INVALID_ARG = 3
ERR_BAD_QUATERNION = 4
ERR_NO_DEVICE = 5
ERR_HIP = 6
ERR_LINE_SEARCH = 7

STATUS_CONVERGED_EXPECTED = 0
STATUS_CONVERGED = 1
STATUS_MAX_ITERS = 2
STATUS_LINE_SEARCH_FAILED = 3
STATUS_QP_FAILED = 4  # extension: a knot's box QP broke down (set_control_limits)
MAX_OBSTACLES = 64  # QILQR_MAX_OBSTACLES: spheres per handle (set_obstacles), and per problem (set_batch_obstacles)
OBSTACLE_WORDS = 8  # QILQR_OBSTACLE_WORDS: {cx, cy, cz, vx, vy, vz, radius, weight} of a per-problem sphere (set_batch_obstacles)
STATE = 13  # QILQR_STATE: words 1..13 of a knot, t(3), q w,x,y,z, v_lin(3), v_ang(3) (shift's x0)
TAILS = {"hold": 0, "hover": 1}  # QILQR_TAIL_HOLD, QILQR_TAIL_HOVER: the control of the knots a shift appends
CL_SCORE = 4  # QILQR_CL_SCORE: cost, min clearance, knot of the min clearance, knots in collision (closed_loop with score=True)
WRENCH = 6  # QILQR_WRENCH: F_x, F_y, F_z (world frame, N), tau_x, tau_y, tau_z (body frame, N m) of a disturbance (closed_loop's wrench)
MC_SUMMARY = 8  # QILQR_MC_SUMMARY: mean cost, its deviation, worst cost, its sample, collision fraction, min clearance, its sample, diverged fraction
RISK = 4  # QILQR_MC_RISK: per level the order statistic (VaR), the mean of the tail behind it (CVaR), the sample at the rank, the tail's count
RISK_MAX_LEVELS = 8  # QILQR_RISK_MAX_LEVELS
RISK_MAX_SAMPLES = 4096  # QILQR_RISK_MAX_SAMPLES: one block sorts a plan's samples
RISK_COLUMNS = {"cost": 0, "clearance": 1}  # QILQR_RISK_COST, QILQR_RISK_CLEARANCE
SELECT_INFO = 4  # QILQR_SELECT_INFO: the chosen objective, the number of feasible candidates, the chosen collision fraction, 1.0 if the fallback chose
SELECT_OBJECTIVES = {"mean": 0, "worst": 1, "var": 2, "cvar": 3}  # qilqr_select_rule.objective: summary words 0 and 2, risk words 0 and 1
MPPI_INFO = 8  # QILQR_MPPI_INFO: J_min, its sample, the effective sample size, the finite samples, the four score words of the new plan (mppi_update_device)
MPPI_FIRST_IS_NOMINAL = 1  # QILQR_MPPI_FIRST_IS_NOMINAL: qilqr_mppi_rule.flags, sample 0 flies the plan's own controls
COV = 144  # QILQR_COV: a knot's covariance, 12 x 12 row-major over the tangent [rho, theta, dv, dw] (covariance_device)
COV_SUMMARY = 8  # QILQR_COV_SUMMARY: max sqrt(tr P), its knot, sqrt(tr P) at the last knot, max rotation deviation, smallest clearance z, its knot, its sphere, max control deviation
COV_WRENCH_HELD = 1  # QILQR_COV_WRENCH_HELD: qilqr_cov_rule.flags, one wrench per flight
FLEET_MAX_NEIGHBOURS = 16  # QILQR_FLEET_MAX_NEIGHBOURS: the K of fleet_neighbours_device
FLEET_NBR = 4  # QILQR_FLEET_NBR: per list entry the partner's row, the smallest distance over the horizon, its knot, the partner's fit residual
FLEET_SUMMARY = 8  # QILQR_FLEET_SUMMARY: smallest distance, its knot, its partner, partners in conflict, spheres written, largest radius written, 0, 0
FLEET_COVER, FLEET_YIELD_TO_LOWER = 1, 2  # QILQR_FLEET_COVER, QILQR_FLEET_YIELD_TO_LOWER: qilqr_fleet_rule.flags
ROUND_KERNELS = 15  # QILQR_ROUND_KERNELS: the k_round instantiations (round_launches)
CL_STATS = 4  # QILQR_CL_STATS: max position error, max rotation error, |dx| at the last knot, clamped (knot, rotor) pairs (closed_loop)

# every symbol include/quadrotor_ilqr.h declares
EXPORTS = (
    "qilqr_create", "qilqr_create_sized", "qilqr_destroy", "qilqr_last_error", "qilqr_solve", "qilqr_solve_batch",
    "qilqr_solve_batch_device", "qilqr_cost_trajectory", "qilqr_backwards_pass", "qilqr_forward_sim",
    "qilqr_line_search", "qilqr_cost_history", "qilqr_profile_reset", "qilqr_profile_get", "qilqr_profile_mode", "qilqr_set_regularisation",
    "qilqr_set_integrator", "qilqr_set_control_limits", "qilqr_set_batch_models", "qilqr_sharded_set_batch_models",
    "qilqr_set_obstacles", "qilqr_sharded_set_obstacles", "qilqr_set_batch_obstacles", "qilqr_sharded_set_batch_obstacles",
    "qilqr_set_state_weight_schedule", "qilqr_sharded_set_state_weight_schedule",
    "qilqr_set_horizon_start", "qilqr_sharded_set_horizon_start", "qilqr_shift_batch", "qilqr_shift_batch_device",
    "qilqr_backwards_pass_device", "qilqr_closed_loop", "qilqr_closed_loop_device",
    "qilqr_closed_loop_scored", "qilqr_closed_loop_scored_device",
    "qilqr_sample_gusts_device", "qilqr_sample_states_device", "qilqr_reduce_scores_device",
    "qilqr_risk_scores_device", "qilqr_select_plans_device",
    "qilqr_mppi_flight_device", "qilqr_mppi_update_device", "qilqr_mppi_flight_spread_device", "qilqr_mppi_adapt_device",
    "qilqr_covariance_device", "qilqr_set_batch_obstacles_device", "qilqr_fleet_neighbours_device",
    "qilqr_device", "qilqr_stream", "qilqr_stream_wait_event", "qilqr_host_alloc", "qilqr_host_free",
    "qilqr_sharded_create", "qilqr_sharded_create_sized", "qilqr_sharded_create_mask", "qilqr_sharded_create_mask_sized", "qilqr_sharded_destroy", "qilqr_sharded_count", "qilqr_sharded_solver",
    "qilqr_shard_range", "qilqr_solve_batch_sharded",
    "qilqr_sharded_set_transport", "qilqr_sharded_transport", "qilqr_solve_batch_sharded_device", "qilqr_gather_schedule",
    "qilqr_abi_version", "qilqr_compaction_moves", "qilqr_describe", "qilqr_round_launches",
)


class Model(C.Structure):
    _fields_ = [("mass_kg", C.c_double), ("inertia", C.c_double * 9), ("arm_length_m", C.c_double),
                ("torque_to_thrust_ratio_m", C.c_double), ("g_mpss", C.c_double)]


class Options(C.Structure):
    _fields_ = [("step_update", C.c_double), ("desired_reduction_frac", C.c_double),
                ("ls_max_iters", C.c_int32), ("rtol", C.c_double), ("atol", C.c_double),
                ("max_iters", C.c_double), ("populate_debug", C.c_int32)]


class DeviceConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("profile", C.c_int32), ("sync_every", C.c_int32),
                ("force_general", C.c_int32), ("single_wave_rollout", C.c_int32), ("precision", C.c_int32),
                ("streams", C.c_int32), ("persistent", C.c_int32), ("compaction", C.c_int32),
                # ABI version 7: the A/B switches that were environment variables
                ("round_launch", C.c_int32), ("rounds_per_launch", C.c_int32), ("fuse_in_flight", C.c_int32), ("dense_weights", C.c_int32)]


class GustModel(C.Structure):
    _fields_ = [("mean", C.c_double * 6), ("sigma", C.c_double * 6), ("tau_force_s", C.c_double), ("tau_torque_s", C.c_double)]


class SelectRule(C.Structure):
    _fields_ = [("objective", C.c_int32), ("level", C.c_int32), ("max_collision_fraction", C.c_double), ("max_diverged_fraction", C.c_double),
                ("min_clearance", C.c_double)]


class MppiRule(C.Structure):
    _fields_ = [("sigma", C.c_double * 4), ("tau_s", C.c_double), ("lambda_", C.c_double), ("collision_cost", C.c_double), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class MppiAdaptRule(C.Structure):
    _fields_ = [("floor", C.c_double * 4), ("cap", C.c_double * 4), ("rate", C.c_double), ("reserved", C.c_double * 3)]


class CovRule(C.Structure):
    _fields_ = [("state_sigma", C.c_double * 12), ("gust", GustModel), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class FleetRule(C.Structure):
    _fields_ = [("radius", C.c_double), ("weight", C.c_double), ("range", C.c_double), ("conflict", C.c_double), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class Profile(C.Structure):
    _fields_ = [("backward_ms", C.c_double), ("backward_launches", C.c_int32),
                ("rollout_ms", C.c_double), ("rollout_launches", C.c_int32),
                ("linearize_ms", C.c_double), ("linearize_launches", C.c_int32),
                ("other_ms", C.c_double), ("other_launches", C.c_int32),
                ("backward_seen", C.c_int32), ("rollout_seen", C.c_int32), ("linearize_seen", C.c_int32),
                ("other_seen", C.c_int32), ("solve_ms", C.c_double), ("solve_launches", C.c_int32), ("solve_seen", C.c_int32)]


_lib = None


def load():
    """Load the HIP library; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        lib.qilqr_last_error.restype = C.c_char_p
        lib.qilqr_stream.restype = C.c_void_p
        lib.qilqr_host_alloc.restype = C.c_void_p
        lib.qilqr_host_alloc.argtypes = [C.c_size_t]
        lib.qilqr_host_free.argtypes = [C.c_void_p]
        lib.qilqr_sharded_solver.restype = C.c_void_p
        lib.qilqr_sharded_solver.argtypes = [C.c_void_p, C.c_int32]
        lib.qilqr_sharded_destroy.argtypes = [C.c_void_p]
        lib.qilqr_sharded_count.argtypes = [C.c_void_p]
        lib.qilqr_sharded_set_transport.argtypes = [C.c_void_p, C.c_int32]
        lib.qilqr_sharded_transport.argtypes = [C.c_void_p]
        lib.qilqr_sharded_transport.restype = C.c_char_p
        lib.qilqr_set_control_limits.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        lib.qilqr_set_batch_models.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.qilqr_sharded_set_batch_models.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.qilqr_set_obstacles.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
        lib.qilqr_sharded_set_obstacles.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
        for f in (lib.qilqr_set_batch_obstacles, lib.qilqr_sharded_set_batch_obstacles):
            f.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32, C.c_int32]
        for f in (lib.qilqr_set_state_weight_schedule, lib.qilqr_sharded_set_state_weight_schedule):
            f.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
        for f in (lib.qilqr_set_horizon_start, lib.qilqr_sharded_set_horizon_start):
            f.argtypes = [C.c_void_p, C.c_int32]
        for f in (lib.qilqr_shift_batch, lib.qilqr_shift_batch_device):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        lib.qilqr_backwards_pass_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        for f in (lib.qilqr_closed_loop, lib.qilqr_closed_loop_device):
            f.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p] * 2
        for f in (lib.qilqr_closed_loop_scored, lib.qilqr_closed_loop_scored_device):
            f.argtypes = [C.c_void_p] * 5 + [C.c_int32, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p] * 3
        lib.qilqr_sample_gusts_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_int32] * 5 + [C.c_void_p]
        lib.qilqr_sample_states_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_int32] * 4 + [C.c_uint32, C.c_void_p]
        lib.qilqr_reduce_scores_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.qilqr_risk_scores_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        lib.qilqr_select_plans_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + \
            [C.c_int32, C.c_void_p, C.c_void_p]
        lib.qilqr_mppi_flight_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p]
        lib.qilqr_mppi_update_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p] * 2
        lib.qilqr_mppi_flight_spread_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p]
        lib.qilqr_mppi_adapt_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p] * 3
        lib.qilqr_covariance_device.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p] * 3
        lib.qilqr_set_batch_obstacles_device.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p]
        lib.qilqr_fleet_neighbours_device.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p] * 4
        _lib = lib
    return _lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _d16(a):
    """_d, on a 16-byte boundary (a row of a larger array may start 8 bytes off one: copied)"""
    a = _d(a)
    return a if a.ctypes.data % 16 == 0 else a.copy()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _raise(rc, ls_max_iters=None):
    msg = load().qilqr_last_error().decode()
    if rc == ERR_BAD_INERTIA:
        raise RuntimeError("Inertia matrix is not positive definite!")  # quadrotor_model.cc:23
    if rc == ERR_LENGTH_MISMATCH:
        raise IndexError(msg)  # std::out_of_range from .at(i), cost.hh:39-40
    if rc == ERR_BAD_QUATERNION:
        raise ValueError(msg)
    if rc == ERR_LINE_SEARCH:
        raise RuntimeError(msg)  # ilqr.hh:191-193, same text
    if rc == ERR_INVALID_ARG:
        raise TypeError(msg)
    raise RuntimeError(f"quadrotor_ilqr error {rc}: {msg}")


def _check(rc, raiser=_raise):
    """every call's return code goes through here: `raiser` turns one that is not OK into the exception"""
    if rc:
        raiser(rc)


def _create_args(self, mass_kg, inertia, arm_length_m, torque_to_thrust_ratio_m, g_mpss, Q, R, desired, options, device, profile,
                 sync_every, force_general, single_wave_rollout, precision, streams, persistent, compaction=0, round_launch=0,
                 rounds_per_launch=0, fuse_in_flight=0, dense_weights=0):
    """the C structures of qilqr_create / qilqr_sharded_create; sets self.options and self.desired"""
    m = Model()
    m.mass_kg = mass_kg
    I = _d(inertia)
    if I.shape != (3, 3):
        raise TypeError("inertia must be 3x3")
    for i in range(9):
        m.inertia[i] = I.reshape(9)[i]
    m.arm_length_m = arm_length_m
    m.torque_to_thrust_ratio_m = torque_to_thrust_ratio_m
    m.g_mpss = g_mpss
    Q, R = _d(Q), _d(R)
    if Q.shape != (12, 12) or R.shape != (4, 4):
        raise TypeError("Q must be 12x12 and R 4x4")
    o = Options()
    o.step_update = options["step_update"]
    o.desired_reduction_frac = options["desired_reduction_frac"]
    o.ls_max_iters = int(options["ls_max_iters"])
    o.rtol = options["rtol"]
    o.atol = options["atol"]
    o.max_iters = float(options["max_iters"])
    o.populate_debug = int(bool(options.get("populate_debug", False)))
    self.options = dict(options)
    self.desired = _d(desired).reshape(-1, KNOT)
    dc = DeviceConfig(int(device), int(profile), int(sync_every), int(force_general),
                      int(single_wave_rollout), {"f64": 0, "f32": 1}[precision], int(streams), int(persistent), int(compaction),
                      int(round_launch), int(rounds_per_launch), int(fuse_in_flight), int(dense_weights))
    return m, Q, R, o, dc


MODEL_FIELDS = ("mass_kg", "inertia", "arm_length_m", "torque_to_thrust_ratio_m", "g_mpss")


def model_array(models):
    """qilqr_model[B] for qilqr_set_batch_models: a sequence of dicts shaped like problems.MODEL_D, or a dict of arrays mass_kg[B],
    inertia[B, 3, 3], arm_length_m[B], torque_to_thrust_ratio_m[B], g_mpss[B] (scalars, and one 3x3 inertia, broadcast)."""
    if isinstance(models, dict):
        cols = {k: np.asarray(models[k], dtype=np.float64) for k in MODEL_FIELDS}
        if cols["inertia"].shape[-2:] != (3, 3):
            raise TypeError("inertia must be 3x3 or [B, 3, 3]")
        lead = [cols[k].shape for k in MODEL_FIELDS if k != "inertia"] + [cols["inertia"].shape[:-2]]
        try:
            shape = np.broadcast_shapes(*lead)
        except ValueError as e:
            raise TypeError(f"model arrays do not broadcast to one batch: {lead}") from e
        if len(shape) != 1:
            raise TypeError("the model arrays must be one-dimensional over the batch (a scalar broadcasts)")
        B = shape[0]
        cols = {k: np.broadcast_to(v, (B, 3, 3) if k == "inertia" else (B,)) for k, v in cols.items()}
    else:
        models = list(models)
        B = len(models)
        cols = {k: np.array([m[k] for m in models], dtype=np.float64).reshape((B, 3, 3) if k == "inertia" else (B,)) for k in MODEL_FIELDS}
    if B == 0:
        raise TypeError("no models: clear_models() switches the per-problem models off")
    arr = (Model * B)()
    for b in range(B):
        m = arr[b]
        m.mass_kg = cols["mass_kg"][b]
        for i, v in enumerate(cols["inertia"][b].reshape(9)):
            m.inertia[i] = v
        m.arm_length_m = cols["arm_length_m"][b]
        m.torque_to_thrust_ratio_m = cols["torque_to_thrust_ratio_m"][b]
        m.g_mpss = cols["g_mpss"][b]
    return arr


def obstacle_array(spheres):
    """(K, 5) float64 rows {cx, cy, cz, radius, weight} for qilqr_set_obstacles (the library checks the values)"""
    arr = _d(spheres)
    if arr.ndim != 2 or arr.shape[1] != 5 or arr.shape[0] == 0:
        raise TypeError(f"obstacles: a (K, 5) array of spheres {{cx, cy, cz, radius, weight}}, K >= 1; got shape {arr.shape} "
                        "(clear_obstacles() switches them off)")
    return arr


def batch_obstacle_arrays(spheres, counts=None):
    """(B, K, 8) float64 spheres {cx, cy, cz, vx, vy, vz, radius, weight} and int32[B] counts (or None) for qilqr_set_batch_obstacles;
    (B, K, 5) rows {cx, cy, cz, radius, weight} are static spheres (v = 0).  The library checks the values."""
    arr = np.asarray(spheres, dtype=np.float64)
    if arr.ndim != 3 or arr.shape[2] not in (5, OBSTACLE_WORDS) or arr.shape[0] == 0 or arr.shape[1] == 0:
        raise TypeError(f"batch obstacles: a (B, K, 8) array {{cx, cy, cz, vx, vy, vz, radius, weight}} or a (B, K, 5) array of static "
                        f"spheres {{cx, cy, cz, radius, weight}}, B, K >= 1; got shape {arr.shape} (clear_batch_obstacles() switches them off)")
    if arr.shape[2] == 5:
        full = np.zeros(arr.shape[:2] + (OBSTACLE_WORDS,))
        full[..., :3] = arr[..., :3]
        full[..., 6:] = arr[..., 3:]
        arr = full
    arr = _d(arr)
    if counts is not None:
        counts = np.asarray(counts)
        if counts.shape != (arr.shape[0],) or not np.issubdtype(counts.dtype, np.integer):
            raise TypeError(f"batch obstacles: counts must be {arr.shape[0]} integers, one per problem; got {counts.dtype} {counts.shape}")
        counts = np.ascontiguousarray(counts, dtype=np.int32)
    return arr, counts


def schedule_array(Qs):
    """(n, 12, 12) float64 state weights for qilqr_set_state_weight_schedule (the library checks the values)"""
    arr = _d(Qs)
    if arr.ndim != 3 or arr.shape[1:] != (12, 12) or arr.shape[0] == 0:
        raise TypeError(f"state-weight schedule: an (n, 12, 12) array of per-knot Q, n >= 1; got shape {arr.shape} "
                        "(clear_state_weight_schedule() switches it off)")
    return arr


def gust_model(sigma, mean=None, tau_force_s=0.0, tau_torque_s=0.0):
    """a qilqr_gust_model: sigma and mean are 6 words {F_x, F_y, F_z, tau_x, tau_y, tau_z}, or two ({force, torque}: the same for x, y, z),
    or one number for all six; tau 0 is white noise per step"""
    def six(v, name):
        v = np.atleast_1d(np.asarray(v, dtype=np.float64))
        if v.shape == (1,):
            v = np.repeat(v, 6)
        elif v.shape == (2,):
            v = np.repeat(v, 3)
        if v.shape != (6,):
            raise TypeError(f"{name} must have 1, 2 or 6 words")
        return v
    m = GustModel()
    m.sigma[:] = six(sigma, "sigma")
    m.mean[:] = six(0.0 if mean is None else mean, "mean")
    m.tau_force_s, m.tau_torque_s = float(tau_force_s), float(tau_torque_s)
    return m


def mppi_rule(sigma, lambda_, tau_s=0.0, collision_cost=0.0, first_is_nominal=True):
    """a qilqr_mppi_rule: sigma one number for the four rotors or four, N; lambda_ the temperature of the weights"""
    sig = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    sig = np.repeat(sig, 4) if sig.shape == (1,) else sig
    if sig.shape != (4,):
        raise TypeError("sigma must have 1 or 4 words")
    return MppiRule((C.c_double * 4)(*sig), float(tau_s), float(lambda_), float(collision_cost), MPPI_FIRST_IS_NOMINAL if first_is_nominal else 0, 0)


def mppi_adapt_rule(floor, cap, rate):
    """a qilqr_mppi_adapt_rule: floor and cap one number for the four rotors or four, N; rate in (0, 1]"""
    def four(v, name):
        v = np.atleast_1d(np.asarray(v, dtype=np.float64))
        v = np.repeat(v, 4) if v.shape == (1,) else v
        if v.shape != (4,):
            raise TypeError(f"{name} must have 1 or 4 words")
        return (C.c_double * 4)(*v)
    return MppiAdaptRule(four(floor, "floor"), four(cap, "cap"), float(rate), (C.c_double * 3)(0.0, 0.0, 0.0))


def cov_rule(state_sigma, gust=None, wrench_held=False):
    """a qilqr_cov_rule: state_sigma 12 words over the tangent [rho, theta, dv, dw] (or one number for all); gust None (no disturbance), a
    GustModel, or a dict with the fields of gust_model (sigma, and optionally mean, tau_force_s, tau_torque_s); wrench_held: one wrench
    per flight (QILQR_COV_WRENCH_HELD)"""
    sig = np.atleast_1d(np.asarray(state_sigma, dtype=np.float64))
    sig = np.repeat(sig, 12) if sig.shape == (1,) else sig
    if sig.shape != (12,):
        raise TypeError("state_sigma must have 1 or 12 words")
    if gust is None:
        gust = gust_model(0.0)
    elif not isinstance(gust, GustModel):
        gust = gust_model(**gust)
    return CovRule((C.c_double * 12)(*sig), gust, COV_WRENCH_HELD if wrench_held else 0, 0)


def fleet_rule(radius, weight, range=np.inf, conflict=None, cover=False, yield_to_lower=False):
    """a qilqr_fleet_rule: a neighbour becomes a sphere of `radius` (plus its fit residual with cover=True) and `weight` if its smallest
    distance over the horizon is below `range`; partners closer than `conflict` (None: radius) are counted in the summary;
    yield_to_lower: only partners in a smaller row are candidates (QILQR_FLEET_YIELD_TO_LOWER)"""
    return FleetRule(float(radius), float(weight), float(range), float(radius if conflict is None else conflict),
                     (FLEET_COVER if cover else 0) | (FLEET_YIELD_TO_LOWER if yield_to_lower else 0), 0)


def _tail(tail):
    if tail not in TAILS:
        raise TypeError(f"tail must be one of {sorted(TAILS)}, not {tail!r}")
    return TAILS[tail]


def _raise_models(rc):
    """_raise, with the index of the first bad model kept in the message (the reference's text, then the problem)"""
    if rc == ERR_BAD_INERTIA:
        raise RuntimeError(load().qilqr_last_error().decode())
    _raise(rc)


def _raise_regularisation(rc):
    if rc == ERR_INVALID_ARG:
        raise ValueError(load().qilqr_last_error().decode())
    _raise(rc)


def _batch_outputs(init, out):
    """result arrays of a batch solve: fresh, or the caller's (checked)"""
    B = init.shape[0]
    if out is None:
        return dict(traj=np.zeros_like(init), cost=np.zeros(B), **{k: np.zeros(B, dtype=np.int32) for k in ("status", "iters", "n_bwd", "n_fwd")})
    for k, dt, shape in (("traj", np.float64, init.shape), ("cost", np.float64, (B,)), ("status", np.int32, (B,)),
                         ("iters", np.int32, (B,)), ("n_bwd", np.int32, (B,)), ("n_fwd", np.int32, (B,))):
        a = out[k]
        if a.dtype != dt or a.shape != shape or not a.flags["C_CONTIGUOUS"]:
            raise TypeError(f"out[{k!r}] must be a C-contiguous {np.dtype(dt).name} array of shape {shape}")
    return out


class QuadrotorILQRBatch:
    """ILQR<QuadrotorModel> (ilqr.hh:25-41) for batches of independent problems on one MI355X."""

    def __init__(self, mass_kg, inertia, arm_length_m, torque_to_thrust_ratio_m, g_mpss, Q, R, desired,
                 dt_s, options, device=0, profile=0, sync_every=2, force_general=False,
                 single_wave_rollout=False, precision="f64", streams=0, persistent=0, compaction=0, round_launch=0,
                 rounds_per_launch=0, fuse_in_flight=0, dense_weights=0):
        lib = load()
        m, Q, R, o, dc = _create_args(self, mass_kg, inertia, arm_length_m, torque_to_thrust_ratio_m, g_mpss, Q, R, desired, options,
                                      device, profile, sync_every, force_general, single_wave_rollout, precision, streams, persistent, compaction,
                                      round_launch, rounds_per_launch, fuse_in_flight, dense_weights)
        self._h = C.c_void_p()
        rc = lib.qilqr_create_sized(C.byref(m), _p(Q), _p(R), _p(self.desired), C.c_int32(len(self.desired)),
                                    C.c_double(dt_s), C.byref(o), C.byref(dc), C.c_size_t(C.sizeof(dc)), C.byref(self._h))
        if rc:
            self._h = None
        _check(rc)

    def close(self):
        if getattr(self, "_h", None):
            load().qilqr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- ILQR::solve, one problem (ilqr.hh:53-87) -> (traj, dict(cost, status, iters, debug...))
    def solve(self, init):
        init = _d(init).reshape(-1, KNOT)
        n = len(init)
        out = np.zeros_like(init)
        # the loop of ilqr.hh:58 runs while i < max_iters with max_iters a double: ceil(max_iters) entries at most
        cap = int(min(max(math.ceil(self.options["max_iters"]), 0), 1e6)) if self.options.get("populate_debug") else 0
        dcost = np.zeros(max(cap, 1))
        dtraj = np.zeros((max(cap, 1), n, KNOT))
        cost, st, it, nd = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(load().qilqr_solve(self._h, _p(init), C.c_int32(n), _p(out), C.byref(cost), C.byref(st),
                                  C.byref(it), _p(dcost), _p(dtraj), C.c_int32(cap), C.byref(nd)))
        k = nd.value
        return out, dict(cost=cost.value, status=st.value, iters=it.value, debug_costs=dcost[:k].copy(),
                         debug_trajs=dtraj[:k].copy())

    # ---- batch of problems, host buffers
    def solve_batch(self, init, desired_batch=None, out=None):
        """qilqr_solve_batch.  `out` (optional): a dict of preallocated result arrays (keys traj, cost, status, iters,
        n_bwd, n_fwd; C-contiguous float64 / int32) that is filled and returned -- with pinned arrays (host_array) the
        copies are direct DMA."""
        init = _d(init)
        B, n = init.shape[0], init.shape[1]
        des = None if desired_batch is None else _d(desired_batch)
        out = _batch_outputs(init, out)
        _check(load().qilqr_solve_batch(self._h, _p(init), _p(des), C.c_int32(B), C.c_int32(n), _p(out["traj"]), _p(out["cost"]),
                                        _ip(out["status"]), _ip(out["iters"]), _ip(out["n_bwd"]), _ip(out["n_fwd"])))
        return out

    # ---- batch of problems, torch CUDA tensors already resident in HBM
    def solve_batch_device(self, init, out_traj, out_cost, out_status, out_iters, out_n_bwd, out_n_fwd,
                           desired_batch=None, wait_current_stream=True):
        """qilqr_solve_batch_device on torch tensors.  Every tensor must live on the solver's device, be
        contiguous and have the ABI's dtype and shape (float64 (B,n,18) / (B,), int32 (B,)); outputs may be None.
        The solve runs on the solver's own stream: it is ordered behind whatever torch has enqueued on its
        current stream (an event recorded here, waited for on the device), and has finished when this returns.
        wait_current_stream=False skips that ordering: only for inputs that are known to be complete (bench.py:
        static inputs, and a gather of the OTHER buffer set still in flight on torch's stream)."""
        import torch
        if init.dim() != 3 or init.shape[2] != KNOT:
            raise TypeError("init must be (B, n, 18)")
        B, n = int(init.shape[0]), int(init.shape[1])
        self._device_tensors(((init, "init", (B, n, KNOT)), (desired_batch, "desired_batch", (B, n, KNOT)), (out_traj, "out_traj", (B, n, KNOT)),
                              (out_cost, "out_cost", (B,))) +
                             tuple((t, name, (B,), torch.int32) for t, name in ((out_status, "out_status"), (out_iters, "out_iters"),
                                                                                (out_n_bwd, "out_n_bwd"), (out_n_fwd, "out_n_fwd"))))
        # inputs produced by asynchronous torch work on its current stream: the solver's stream waits for them
        if wait_current_stream:
            self._wait_current_stream(init)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_solve_batch_device(self._h, vp(init), vp(desired_batch), C.c_int32(B), C.c_int32(n),
                                               vp(out_traj), vp(out_cost), vp(out_status), vp(out_iters),
                                               vp(out_n_bwd), vp(out_n_fwd)))

    # ---- the passes the reference tests individually (ilqr_test.cc:102-190), batched
    def cost_trajectory(self, traj):
        traj = _d(traj)
        B, n = traj.shape[0], traj.shape[1]
        cost = np.zeros(B)
        _check(load().qilqr_cost_trajectory(self._h, _p(traj), C.c_int32(B), C.c_int32(n), _p(cost)))
        return cost

    def backwards_pass(self, traj):
        traj = _d(traj)
        B, n = traj.shape[0], traj.shape[1]
        gains = np.zeros((B, n, GAIN))
        terms = np.zeros((B, 2))
        _check(load().qilqr_backwards_pass(self._h, _p(traj), C.c_int32(B), C.c_int32(n), _p(gains), _p(terms)))
        return gains, terms

    def forward_sim(self, traj, gains, alpha=1.0):
        traj, gains = _d(traj), _d(gains)
        B, n = traj.shape[0], traj.shape[1]
        alpha = _d(np.broadcast_to(alpha, (B,)))
        out = np.zeros_like(traj)
        _check(load().qilqr_forward_sim(self._h, _p(traj), _p(gains), _p(alpha), C.c_int32(B), C.c_int32(n), _p(out)))
        return out

    def line_search(self, traj, cost, gains, terms):
        traj, gains, cost, terms = _d(traj), _d(gains), _d(cost), _d(terms)
        B, n = traj.shape[0], traj.shape[1]
        out = np.zeros_like(traj)
        oc, step = np.zeros(B), np.zeros(B)
        st = np.zeros(B, dtype=np.int32)
        _check(load().qilqr_line_search(self._h, _p(traj), _p(cost), _p(gains), _p(terms), C.c_int32(B), C.c_int32(n),
                                        _p(out), _p(oc), _p(step), _ip(st)))
        return dict(traj=out, cost=oc, step=step, status=st)

    def cost_history(self, B):
        """(B, cap) array: cost after every completed forward pass of the last batch solve (NaN padded);
        needs options['populate_debug']"""
        cap = C.c_int32()
        load().qilqr_cost_history(self._h, C.c_int32(B), None, C.c_int32(0), C.byref(cap))
        hist = np.zeros((B, max(cap.value, 1)))
        _check(load().qilqr_cost_history(self._h, C.c_int32(B), _p(hist), C.c_int32(hist.shape[1]), C.byref(cap)))
        return hist

    # ---- profiling
    def profile_reset(self):
        _check(load().qilqr_profile_reset(self._h))

    def profile_mode(self, mode):
        """0 off, 1 k_backward + k_rollout, 2 every kernel, 3 k_backward only, 4 k_rollout only"""
        _check(load().qilqr_profile_mode(self._h, C.c_int32(int(mode))))

    def describe(self, B):
        """qilqr_describe: in words, the arithmetic and the kernels a batch solve of B problems on this handle uses"""
        buf = C.create_string_buffer(2048)
        _check(load().qilqr_describe(self._h, C.c_int32(int(B)), buf, C.c_size_t(len(buf))))
        return buf.value.decode()

    def compaction_moves(self):
        """trajectories the compaction moved in the last batch solve (qilqr_compaction_moves)"""
        m = C.c_int64()
        _check(load().qilqr_compaction_moves(self._h, C.byref(m)))
        return m.value

    def set_regularisation(self, mu_init, mu_factor=10.0, mu_max=1e6):
        """Levenberg-Marquardt restarts (an extension the reference lacks; mu_init = 0 switches it off):
        see qilqr_set_regularisation in include/quadrotor_ilqr.h"""
        _check(load().qilqr_set_regularisation(self._h, C.c_double(mu_init), C.c_double(mu_factor), C.c_double(mu_max)), _raise_regularisation)

    def set_integrator(self, integrator):
        """Runge-Kutta extension (the step sketched at quadrotor_model.cc:51-63; 0 = the reference's explicit Euler)."""
        _check(load().qilqr_set_integrator(self._h, C.c_int32(int(integrator))))

    def set_control_limits(self, lo, hi):
        """Per-rotor thrust limits lo <= u_a <= hi (N; scalars or four values, +-inf leaves a side open) -- an extension: box-constrained
        iLQR, see qilqr_set_control_limits in include/quadrotor_ilqr.h.  clear_control_limits() switches it off again."""
        lo = _d(np.broadcast_to(np.asarray(lo, dtype=np.float64), (4,)))
        hi = _d(np.broadcast_to(np.asarray(hi, dtype=np.float64), (4,)))
        _check(load().qilqr_set_control_limits(self._h, _p(lo), _p(hi)))

    def clear_control_limits(self):
        _check(load().qilqr_set_control_limits(self._h, None, None))

    def set_models(self, models):
        """Per-problem models (an extension): problem b of every batch entry point is solved with models[b] -- see model_array for the
        forms `models` takes, and qilqr_set_batch_models in include/quadrotor_ilqr.h.  Every call is then over exactly that many
        problems.  clear_models() switches it off again."""
        arr = model_array(models)
        _check(load().qilqr_set_batch_models(self._h, C.cast(arr, C.c_void_p), C.c_int32(len(arr))), _raise_models)

    def clear_models(self):
        _check(load().qilqr_set_batch_models(self._h, None, C.c_int32(0)))

    def set_obstacles(self, spheres):
        """Spherical obstacles penalised in the cost (an extension): `spheres` is a (K, 5) array of {cx, cy, cz, radius, weight}, K <= 64,
        shared by every problem -- see qilqr_set_obstacles in include/quadrotor_ilqr.h.  clear_obstacles() switches them off again."""
        arr = obstacle_array(spheres)
        _check(load().qilqr_set_obstacles(self._h, _p(arr), C.c_int32(len(arr))))

    def clear_obstacles(self):
        _check(load().qilqr_set_obstacles(self._h, None, C.c_int32(0)))

    def set_batch_obstacles(self, spheres, counts=None):
        """Per-problem, moving spheres (an extension): `spheres` is (B, K, 8) {cx, cy, cz, vx, vy, vz, radius, weight} or (B, K, 5) static
        {cx, cy, cz, radius, weight}; problem b uses its first counts[b] rows (all K without counts).  At knot i the centre is c + i dt v.
        Every call that evaluates the cost is then over exactly B problems -- see qilqr_set_batch_obstacles in include/quadrotor_ilqr.h.
        clear_batch_obstacles() switches them off again."""
        arr, cnt = batch_obstacle_arrays(spheres, counts)
        _check(load().qilqr_set_batch_obstacles(self._h, _p(arr), _ip(cnt), C.c_int32(arr.shape[0]), C.c_int32(arr.shape[1])))

    def clear_batch_obstacles(self):
        _check(load().qilqr_set_batch_obstacles(self._h, None, None, C.c_int32(0), C.c_int32(0)))

    def set_state_weight_schedule(self, Qs):
        """Per-knot state weights (an extension): `Qs` is an (n, 12, 12) array and knot i of every problem takes Qs[i] for Q -- terminal
        and waypoint costs (problems.terminal_schedule, problems.waypoint_schedule); see qilqr_set_state_weight_schedule in
        include/quadrotor_ilqr.h.  clear_state_weight_schedule() switches it off again."""
        arr = schedule_array(Qs)
        _check(load().qilqr_set_state_weight_schedule(self._h, _p(arr), C.c_int32(len(arr))))

    def clear_state_weight_schedule(self):
        _check(load().qilqr_set_state_weight_schedule(self._h, None, C.c_int32(0)))

    # ---- receding-horizon stepping
    def set_horizon_start(self, k0):
        """From this call on knot i of every call reads desired[k0 + i] of the handle's desired trajectory and Qs[k0 + i] of its
        state-weight schedule (an extension; 0 restores the handle) -- see qilqr_set_horizon_start in include/quadrotor_ilqr.h."""
        _check(load().qilqr_set_horizon_start(self._h, C.c_int32(int(k0))))

    def shift(self, traj, x0=None, steps=1, tail="hold"):
        """qilqr_shift_batch, host arrays: the plan (B, n, 18) moved `steps` knots towards its start, its end extended by dynamics steps
        under the held last control (tail='hold') or the hover thrust ('hover'), knot 0's state replaced by x0 (B, 13) when given.  Returns
        the new (B, n, 18) array: the next solve's initial trajectory."""
        traj = _d16(traj)
        if traj.ndim != 3 or traj.shape[2] != KNOT:
            raise TypeError("traj must be (B, n, 18)")
        B, n = traj.shape[0], traj.shape[1]
        if x0 is not None:
            x0 = _d16(x0)
            if x0.shape != (B, STATE):
                raise TypeError(f"x0 must be ({B}, {STATE}): words 1..13 of a knot per problem")
        out = np.zeros_like(traj)
        vp = lambda a: C.c_void_p(0 if a is None else a.ctypes.data)
        _check(load().qilqr_shift_batch(self._h, vp(traj), vp(x0), C.c_int32(B), C.c_int32(n), C.c_int32(int(steps)), C.c_int32(_tail(tail)), vp(out)))
        return out

    def shift_device(self, traj, out, x0=None, steps=1, tail="hold", wait_current_stream=True):
        """qilqr_shift_batch_device on torch tensors, checked like solve_batch_device: traj and out float64 (B, n, 18), x0 float64 (B, 13)
        or None, on the solver's device, contiguous.  The launch is ENQUEUED on the solver's own stream -- behind whatever torch has
        enqueued on its current stream (wait_current_stream) -- and this returns without waiting: a solve on this handle is ordered behind
        it; torch work that reads `out` waits for the solver's stream first (any draining call of the handle, or an event)."""
        if traj.dim() != 3 or traj.shape[2] != KNOT:
            raise TypeError("traj must be (B, n, 18)")
        B, n = int(traj.shape[0]), int(traj.shape[1])
        self._device_tensors(((traj, "traj", (B, n, KNOT)), (out, "out", (B, n, KNOT)), (x0, "x0", (B, STATE))), required=("traj", "out"))
        tail = _tail(tail)
        if wait_current_stream:
            self._wait_current_stream(traj)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_shift_batch_device(self._h, vp(traj), vp(x0), C.c_int32(B), C.c_int32(n), C.c_int32(int(steps)), C.c_int32(tail), vp(out)))

    # ---- the plan's feedback law: gains about a plan on the device, and the law flown from given states
    def _device_tensors(self, specs, required=()):
        """checks of the device entry points: (tensor, name, shape[, dtype]) of that dtype (float64), contiguous, on the solver's device;
        None is skipped unless the name is in `required`"""
        import torch
        dev_index = load().qilqr_device(self._h)
        for t, name, shape, *dtype in specs:
            dtype = dtype[0] if dtype else torch.float64
            if t is None and name not in required:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != dev_index:
                raise TypeError(f"{name} must be a CUDA tensor on device {dev_index}")
            if t.dtype != dtype:
                raise TypeError(f"{name} must be {dtype}")
            if tuple(t.shape) != shape:
                raise TypeError(f"{name} must have shape {shape}, not {tuple(t.shape)}")
            if not t.is_contiguous():
                raise TypeError(f"{name} must be contiguous")

    def _wait_current_stream(self, t):
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(t.device))
        _check(load().qilqr_stream_wait_event(self._h, C.c_void_p(ev.cuda_event)))

    def backwards_pass_device(self, traj, gains, terms=None, wait_current_stream=True):
        """qilqr_backwards_pass_device on torch tensors: traj float64 (B, n, 18) -> gains (B, n, 52) and, when given, terms (B, 2), the bits
        of backwards_pass(traj) without the trip over the host.  Ordered behind torch's current stream (wait_current_stream) and
        finished when this returns, as solve_batch_device."""
        if traj is None or traj.dim() != 3 or traj.shape[2] != KNOT:
            raise TypeError("traj must be (B, n, 18)")
        if gains is None:
            raise TypeError("gains must be a (B, n, 52) tensor")
        B, n = int(traj.shape[0]), int(traj.shape[1])
        self._device_tensors(((traj, "traj", (B, n, KNOT)), (gains, "gains", (B, n, GAIN)), (terms, "terms", (B, 2))))
        if wait_current_stream:
            self._wait_current_stream(traj)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_backwards_pass_device(self._h, vp(traj), C.c_int32(B), C.c_int32(n), vp(gains), vp(terms)))

    def closed_loop(self, plan, gains, x0, i0=0, i1=None, traj=True, stats=True, wrench=None, desired=None, score=False):
        """qilqr_closed_loop, host arrays: the law u = u_i + K_i (x (-) plan_i) of plan (B, n, 18) and gains (B, n, 52) flown from the
        states x0 (B, S, 13) -- or (B, 13): S = 1 -- over knots i0 .. i1 (i1 = None: n - 1) with the handle's step, thrust limits and
        per-problem models (B * S of them: model b S + j flies sample (b, j)).  Returns a dict: traj (B, S, n, 18), NaN outside knots
        i0 .. i1 (traj=True), and stats (B, S, 4): max position error, max rotation error, |dx| at knot i1, clamped (knot, rotor) pairs
        (stats=True).
        wrench, desired, score (without any of them the scored entry point, which is always the one called, is qilqr_closed_loop): wrench (B, S, n_w, 6) -- or
        (B, S, 6): n_w = 1 -- with n_w 1 or n, {F world frame, tau body frame} held over each step; score=True adds score (B, S, 4): the
        handle's cost of the flown knots i0 .. i1, the smallest clearance to any sphere of the handle's two tables, its knot, and the
        number of knots in collision; desired (B, n, 18): the cost is taken against it instead of the handle's desired trajectory."""
        plan, gains, x0 = _d16(plan), _d16(gains), _d16(x0)
        if plan.ndim != 3 or plan.shape[2] != KNOT:
            raise TypeError("plan must be (B, n, 18)")
        B, n = plan.shape[0], plan.shape[1]
        if gains.shape != (B, n, GAIN):
            raise TypeError(f"gains must be ({B}, {n}, {GAIN})")
        if x0.ndim == 2:
            x0 = x0.reshape(x0.shape[0], 1, x0.shape[1])
        if x0.ndim != 3 or x0.shape[0] != B or x0.shape[2] != STATE:
            raise TypeError(f"x0 must be ({B}, S, {STATE}): words 1..13 of a knot per sample")
        S = x0.shape[1]
        i1 = n - 1 if i1 is None else int(i1)
        out_traj = _d16(np.full((B, S, n, KNOT), np.nan)) if traj else None
        out_stats = _d16(np.zeros((B, S, CL_STATS))) if stats else None
        vp = lambda a: C.c_void_p(0 if a is None else a.ctypes.data)
        n_w = 1
        if wrench is not None:
            wrench = _d16(wrench)
            if wrench.ndim == 3:
                wrench = wrench.reshape(wrench.shape[0], wrench.shape[1], 1, wrench.shape[2])
            if wrench.ndim != 4 or wrench.shape[:2] != (B, S) or wrench.shape[3] != WRENCH:
                raise TypeError(f"wrench must be ({B}, {S}, n_w, {WRENCH}) with n_w 1 or n")
            n_w = wrench.shape[2]
        if desired is not None:
            desired = _d16(desired)
            if desired.shape != (B, n, KNOT):
                raise TypeError(f"desired must be ({B}, {n}, {KNOT}): one desired trajectory per plan")
        out_score = _d16(np.zeros((B, S, CL_SCORE))) if score else None
        _check(load().qilqr_closed_loop_scored(self._h, vp(plan), vp(gains), vp(x0), vp(wrench), C.c_int32(n_w), vp(desired), C.c_int32(B), C.c_int32(n),
                                               C.c_int32(S), C.c_int32(int(i0)), C.c_int32(i1), vp(out_traj), vp(out_stats), vp(out_score)))
        return {k: v for k, v in (("traj", out_traj), ("stats", out_stats), ("score", out_score)) if v is not None}

    def closed_loop_device(self, plan, gains, x0, out_traj=None, out_stats=None, i0=0, i1=None, wait_current_stream=True, wrench=None, desired=None,
                           out_score=None):
        """qilqr_closed_loop_device on torch tensors, checked like shift_device: plan (B, n, 18), gains (B, n, 52), x0 (B, S, 13), out_traj
        (B, S, n, 18) or None, out_stats (B, S, 4) or None, float64, contiguous, on the solver's device.  Only knots i0 .. i1 of out_traj
        are written.  ENQUEUED on the solver's own stream -- behind whatever torch has enqueued on its current stream
        (wait_current_stream) -- and not waited for: stream ordering as for shift_device.
        wrench (B, S, n_w, 6), desired (B, n, 18) and out_score (B, S, 4), checked like the others, are qilqr_closed_loop_scored_device's
        (closed_loop's docstring); without any of them that entry point, always the one called, is qilqr_closed_loop_device."""
        if plan is None or plan.dim() != 3 or plan.shape[2] != KNOT:
            raise TypeError("plan must be (B, n, 18)")
        B, n = int(plan.shape[0]), int(plan.shape[1])
        if x0 is None or x0.dim() != 3:
            raise TypeError(f"x0 must be ({B}, S, {STATE})")
        S = int(x0.shape[1])
        i1 = n - 1 if i1 is None else int(i1)
        self._device_tensors(((plan, "plan", (B, n, KNOT)), (gains, "gains", (B, n, GAIN)), (x0, "x0", (B, S, STATE)),
                              (out_traj, "out_traj", (B, S, n, KNOT)), (out_stats, "out_stats", (B, S, CL_STATS))))
        if gains is None:
            raise TypeError("gains must be a (B, n, 52) tensor")
        n_w = 1
        if wrench is not None:
            if wrench.dim() != 4:
                raise TypeError(f"wrench must be ({B}, {S}, n_w, {WRENCH}) with n_w 1 or n")
            n_w = int(wrench.shape[2])
        self._device_tensors(((wrench, "wrench", (B, S, n_w, WRENCH)), (desired, "desired", (B, n, KNOT)), (out_score, "out_score", (B, S, CL_SCORE))))
        if wait_current_stream:
            self._wait_current_stream(plan)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_closed_loop_scored_device(self._h, vp(plan), vp(gains), vp(x0), vp(wrench), C.c_int32(n_w), vp(desired), C.c_int32(B),
                                                      C.c_int32(n), C.c_int32(S), C.c_int32(int(i0)), C.c_int32(i1), vp(out_traj), vp(out_stats),
                                                      vp(out_score)))

    # ---- the ends of the Monte-Carlo loop: gusts and start states sampled, and scores reduced, on the device
    def sample_gusts_device(self, out, seed, sigma, mean=None, tau_force_s=0.0, tau_torque_s=0.0, b0=0, s0=0, wait_current_stream=True):
        """qilqr_sample_gusts_device: fills out (B, S, n_w, 6), a float64 tensor on the solver's device, with Gauss-Markov gusts of
        deviation sigma about mean (gust_model's forms) and correlation times tau_force_s, tau_torque_s (0: white noise per step) -- the
        wrench of closed_loop_device.  A word depends on (seed, b0 + b, s0 + s, knot, component) and the model alone.  ENQUEUED on the
        solver's own stream and not waited for, as closed_loop_device."""
        if out is None or out.dim() != 4:
            raise TypeError(f"out must be (B, S, n_w, {WRENCH})")
        B, S, n_w = (int(v) for v in out.shape[:3])
        self._device_tensors(((out, "out", (B, S, n_w, WRENCH)),))
        m = gust_model(sigma, mean, tau_force_s, tau_torque_s)
        if wait_current_stream:
            self._wait_current_stream(out)
        _check(load().qilqr_sample_gusts_device(self._h, C.byref(m), C.c_uint64(int(seed)), C.c_int32(B), C.c_int32(S), C.c_int32(n_w), C.c_int32(int(b0)),
                                                C.c_int32(int(s0)), C.c_void_p(out.data_ptr())))

    def sample_states_device(self, x_nom, out, seed, sigma, b0=0, s0=0, first_is_nominal=False, wait_current_stream=True):
        """qilqr_sample_states_device: out[b, s] = x_nom[b] (+) sigma * xi, x_nom (B, 13) and out (B, S, 13) float64 tensors on the solver's
        device, sigma 12 words over the tangent [rho, theta, dv, dw] (or one number for all).  first_is_nominal: sample s0 + s == 0 is
        x_nom[b] itself.  ENQUEUED on the solver's own stream and not waited for."""
        if out is None or out.dim() != 3:
            raise TypeError(f"out must be (B, S, {STATE})")
        B, S = int(out.shape[0]), int(out.shape[1])
        self._device_tensors(((x_nom, "x_nom", (B, STATE)), (out, "out", (B, S, STATE))))
        if x_nom is None:
            raise TypeError(f"x_nom must be a ({B}, {STATE}) tensor")
        sig = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
        sig = np.ascontiguousarray(np.repeat(sig, 12) if sig.shape == (1,) else sig)
        if sig.shape != (12,):
            raise TypeError("sigma must have 1 or 12 words")
        if wait_current_stream:
            self._wait_current_stream(out)
        _check(load().qilqr_sample_states_device(self._h, C.c_void_p(x_nom.data_ptr()), C.c_void_p(sig.ctypes.data), C.c_uint64(int(seed)), C.c_int32(B),
                                                 C.c_int32(S), C.c_int32(int(b0)), C.c_int32(int(s0)), C.c_uint32(1 if first_is_nominal else 0),
                                                 C.c_void_p(out.data_ptr())))

    def reduce_scores_device(self, score, out, wait_current_stream=True):
        """qilqr_reduce_scores_device: out (B, 8) from score (B, S, 4) as closed_loop_device's out_score holds it: mean cost, its deviation,
        worst cost, its sample, the fraction in collision, the smallest clearance, its sample, the fraction that diverged.  ENQUEUED on
        the solver's own stream and not waited for."""
        if score is None or score.dim() != 3:
            raise TypeError(f"score must be (B, S, {CL_SCORE})")
        B, S = int(score.shape[0]), int(score.shape[1])
        self._device_tensors(((score, "score", (B, S, CL_SCORE)), (out, "out", (B, MC_SUMMARY))))
        if out is None:
            raise TypeError(f"out must be a ({B}, {MC_SUMMARY}) tensor")
        if wait_current_stream:
            self._wait_current_stream(score)
        _check(load().qilqr_reduce_scores_device(self._h, C.c_void_p(score.data_ptr()), C.c_int32(B), C.c_int32(S), C.c_void_p(out.data_ptr())))

    # ---- behind the reduction: tail measures per plan, and the choice among a vehicle's candidate plans
    def risk_scores_device(self, score, out, levels, column="cost", wait_current_stream=True):
        """qilqr_risk_scores_device: out (B, L, 4) from score (B, S, 4) as closed_loop_device's out_score holds it, S <= 4096: per level of
        `levels` (L <= 8 numbers in [0, 1)) the order statistic of the cost at rank ceil(level S) - 1 (VaR), the mean of the tail from
        there on (CVaR), the sample at the rank and the tail's count; column="clearance": of the clearance, the lower tail (the clearance
        all but the worst flights keep, the mean of the smallest).  A NaN counts as the worst outcome.  ENQUEUED on the solver's own
        stream and not waited for."""
        if score is None or score.dim() != 3:
            raise TypeError(f"score must be (B, S, {CL_SCORE})")
        if column not in RISK_COLUMNS:
            raise TypeError("column must be 'cost' or 'clearance'")
        B, S = int(score.shape[0]), int(score.shape[1])
        lv = np.ascontiguousarray(np.atleast_1d(np.asarray(levels, dtype=np.float64)))
        if lv.ndim != 1 or not 1 <= len(lv) <= RISK_MAX_LEVELS:
            raise TypeError(f"levels must be 1 ... {RISK_MAX_LEVELS} numbers")
        self._device_tensors(((score, "score", (B, S, CL_SCORE)), (out, "out", (B, len(lv), RISK))), required=("out",))
        if wait_current_stream:
            self._wait_current_stream(score)
        _check(load().qilqr_risk_scores_device(self._h, C.c_void_p(score.data_ptr()), C.c_int32(B), C.c_int32(S), C.c_int32(RISK_COLUMNS[column]),
                                               C.c_void_p(lv.ctypes.data), C.c_int32(len(lv)), C.c_void_p(out.data_ptr())))

    def select_plans_device(self, summary, C, choice, info, objective="cvar", level=0, risk=None, max_collision_fraction=1.0, max_diverged_fraction=1.0,
                            min_clearance=-np.inf, plan=None, gains=None, out_plan=None, out_gains=None, wait_current_stream=True):
        """qilqr_select_plans_device: of the C candidate plans of each of V vehicles (summary (C V, 8) from reduce_scores_device, plan
        b = c V + v; risk (C V, L, 4) from risk_scores_device on the cost column) the feasible one -- collision fraction, diverged fraction
        and smallest clearance within the three thresholds, objective not NaN -- with the smallest objective ("mean", "worst": summary words
        0 and 2; "var", "cvar": words 0 and 1 of the risk array's `level`), the smaller candidate on ties; without a feasible one the
        smallest (collision fraction, diverged fraction, objective, c).  choice (V,) int32 and info (V, 4) receive the candidate and
        {its objective, the number of feasible candidates, its collision fraction, 1.0 if the fallback chose}.  plan (C V, n, 18), gains
        (C V, n, 52), out_plan (V, n, 18) and out_gains (V, n, 52), all four or none: the chosen plans and their gains are gathered.
        ENQUEUED on the solver's own stream and not waited for."""
        import ctypes as ct  # (C is the number of candidates here, as in the C ABI)
        import torch
        if summary is None or summary.dim() != 2:
            raise TypeError(f"summary must be (C V, {MC_SUMMARY})")
        cands = int(C)
        if cands <= 0 or int(summary.shape[0]) % cands:
            raise TypeError(f"summary has {int(summary.shape[0])} plans: not a multiple of {cands} candidates")
        if objective not in SELECT_OBJECTIVES:
            raise TypeError("objective must be one of " + ", ".join(SELECT_OBJECTIVES))
        V = int(summary.shape[0]) // cands
        L = 0 if risk is None else (int(risk.shape[1]) if risk.dim() == 3 else -1)
        gather = [t for t in (plan, gains, out_plan, out_gains) if t is not None]
        if len(gather) not in (0, 4):
            raise TypeError("plan, gains, out_plan and out_gains are given all together or not at all")
        n = int(plan.shape[1]) if gather and plan.dim() == 3 else 0
        self._device_tensors(((summary, "summary", (cands * V, MC_SUMMARY)), (risk, "risk", (cands * V, L, RISK)), (choice, "choice", (V,), torch.int32),
                              (info, "info", (V, SELECT_INFO)), (plan, "plan", (cands * V, n, KNOT)), (gains, "gains", (cands * V, n, GAIN)),
                              (out_plan, "out_plan", (V, n, KNOT)), (out_gains, "out_gains", (V, n, GAIN))), required=("choice", "info"))
        rule = SelectRule(SELECT_OBJECTIVES[objective], int(level), float(max_collision_fraction), float(max_diverged_fraction), float(min_clearance))
        if wait_current_stream:
            self._wait_current_stream(summary)
        vp = lambda t: ct.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_select_plans_device(self._h, vp(summary), vp(risk), ct.c_int32(max(L, 0)), ct.byref(rule), ct.c_int32(V), ct.c_int32(cands), vp(choice),
                                                vp(info), vp(plan), vp(gains), ct.c_int32(n), vp(out_plan), vp(out_gains)))

    # ---- the sampling planner: control-perturbed flights of a plan, and the plan moved to their weighted mean
    def _mppi_tensors(self, plan, x0, desired, score):
        if plan is None or plan.dim() != 3 or plan.shape[2] != KNOT:
            raise TypeError("plan must be (B, n, 18)")
        if score is None or score.dim() != 3:
            raise TypeError(f"score must be (B, S, {CL_SCORE})")
        B, n, S = int(plan.shape[0]), int(plan.shape[1]), int(score.shape[1])
        self._device_tensors(((plan, "plan", (B, n, KNOT)), (x0, "x0", (B, STATE)), (desired, "desired", (B, n, KNOT)), (score, "score", (B, S, CL_SCORE))))
        return B, n, S

    def mppi_flight_device(self, plan, score, seed, sigma, lambda_=1.0, tau_s=0.0, collision_cost=0.0, first_is_nominal=True, x0=None, desired=None, b0=0,
                           wait_current_stream=True):
        """qilqr_mppi_flight_device on torch tensors: S = score.shape[1] copies of each plan of plan (B, n, 18) flown open loop from x0 (B, 13;
        None: the plan's knot 0) under u_i = clamp(plan_u_i + eps_i), eps a Gauss-Markov perturbation per rotor of deviation sigma (one
        number or four, N) and correlation time tau_s (0: white) drawn from (seed, b0 + b, sample, knot), and scored as closed_loop_device
        scores a flight (desired (B, n, 18): against it instead of the handle's desired trajectory) into score (B, S, 4) -- what
        reduce_scores_device and risk_scores_device read.  first_is_nominal: sample 0 flies the plan's own controls.  lambda_ and
        collision_cost are the update's and only checked here.  ENQUEUED on the solver's own stream and not waited for."""
        B, n, S = self._mppi_tensors(plan, x0, desired, score)
        rule = mppi_rule(sigma, lambda_, tau_s, collision_cost, first_is_nominal)
        if wait_current_stream:
            self._wait_current_stream(plan)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_mppi_flight_device(self._h, C.byref(rule), C.c_uint64(int(seed)), vp(plan), vp(x0), vp(desired), C.c_int32(B), C.c_int32(n),
                                               C.c_int32(S), C.c_int32(int(b0)), vp(score)))

    def mppi_update_device(self, plan, score, out_plan, info, seed, sigma, lambda_, tau_s=0.0, collision_cost=0.0, first_is_nominal=True, x0=None,
                           desired=None, b0=0, wait_current_stream=True):
        """qilqr_mppi_update_device on torch tensors: from the scores (B, S, 4) of mppi_flight_device called with the same plan, seed, sigma,
        tau_s, first_is_nominal, x0, desired and b0, out_plan (B, n, 18) receives the plan with its controls moved to the weighted mean
        perturbation -- weights exp(-(J - J_min) / lambda_), J = cost + collision_cost * knots in collision, the perturbations redrawn --
        clamped to the thrust limits, and its states flown from x0 under those controls: a trajectory solve_batch_device accepts as its
        initial one.  info (B, 8): J_min, its sample, the effective sample size, the samples with a finite J, and the four score words of the
        new plan.  ENQUEUED on the solver's own stream (two launches) and not waited for."""
        B, n, S = self._mppi_tensors(plan, x0, desired, score)
        self._device_tensors(((out_plan, "out_plan", (B, n, KNOT)), (info, "info", (B, MPPI_INFO))), required=("out_plan", "info"))
        rule = mppi_rule(sigma, lambda_, tau_s, collision_cost, first_is_nominal)
        if wait_current_stream:
            self._wait_current_stream(plan)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_mppi_update_device(self._h, C.byref(rule), C.c_uint64(int(seed)), vp(plan), vp(x0), vp(desired), vp(score), C.c_int32(B),
                                               C.c_int32(n), C.c_int32(S), C.c_int32(int(b0)), vp(out_plan), vp(info)))

    def mppi_flight_spread_device(self, plan, spread, score, seed, sigma, lambda_=1.0, tau_s=0.0, collision_cost=0.0, first_is_nominal=True, x0=None,
                                  desired=None, b0=0, wait_current_stream=True):
        """qilqr_mppi_flight_spread_device on torch tensors: mppi_flight_device with the perturbation's deviation read per plan, knot and
        rotor from spread (B, n, 4), N -- eps = spread * z, z the recursion of unit deviation over the same draws.  sigma is checked as
        before and not read for the draws.  ENQUEUED on the solver's own stream and not waited for."""
        B, n, S = self._mppi_tensors(plan, x0, desired, score)
        self._device_tensors(((spread, "spread", (B, n, 4)),), required=("spread",))
        rule = mppi_rule(sigma, lambda_, tau_s, collision_cost, first_is_nominal)
        if wait_current_stream:
            self._wait_current_stream(plan)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_mppi_flight_spread_device(self._h, C.byref(rule), C.c_uint64(int(seed)), vp(plan), vp(x0), vp(desired), vp(spread), C.c_int32(B),
                                                      C.c_int32(n), C.c_int32(S), C.c_int32(int(b0)), vp(score)))

    def mppi_adapt_device(self, plan, spread, score, out_plan, out_spread, info, seed, sigma, lambda_, floor, cap, rate, tau_s=0.0, collision_cost=0.0,
                          first_is_nominal=True, x0=None, desired=None, b0=0, wait_current_stream=True):
        """qilqr_mppi_adapt_device on torch tensors: mppi_update_device over the scores (B, S, 4) of mppi_flight_spread_device called with
        the same plan, spread, seed, tau_s, first_is_nominal, x0, desired and b0 -- out_plan (B, n, 18) and info (B, 8) as the update
        makes them -- and out_spread (B, n, 4; None: the mean only), the spread blended towards the weighted deviation of the
        perturbations: new variance = (1 - rate) old + rate weighted, its root clamped to [floor, cap] (one number or four, N).  Not in
        place.  ENQUEUED on the solver's own stream (two launches) and not waited for."""
        B, n, S = self._mppi_tensors(plan, x0, desired, score)
        self._device_tensors(((spread, "spread", (B, n, 4)), (out_plan, "out_plan", (B, n, KNOT)), (out_spread, "out_spread", (B, n, 4)),
                              (info, "info", (B, MPPI_INFO))), required=("spread", "out_plan", "info"))
        rule = mppi_rule(sigma, lambda_, tau_s, collision_cost, first_is_nominal)
        adapt = mppi_adapt_rule(floor, cap, rate)
        if wait_current_stream:
            self._wait_current_stream(plan)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_mppi_adapt_device(self._h, C.byref(rule), C.byref(adapt), C.c_uint64(int(seed)), vp(plan), vp(x0), vp(desired), vp(spread),
                                              vp(score), C.c_int32(B), C.c_int32(n), C.c_int32(S), C.c_int32(int(b0)), vp(out_plan), vp(out_spread), vp(info)))

    # ---- linear covariance analysis of a plan's closed loop: the first-order answer to what the Monte-Carlo loop samples
    def covariance_device(self, plan, gains, state_sigma, gust=None, i0=0, i1=None, wrench_held=False, cov=None, mean=None, summary=None,
                          wait_current_stream=True):
        """qilqr_covariance_device on torch tensors: the covariance of the deviation dx_i = x_i (-) plan_i of the law u = u_i + K_i dx over
        knots i0 .. i1 (i1 = None: n - 1) of plan (B, n, 18) with gains (B, n, 52), or None: the open loop -- from a start state with
        deviations state_sigma (12 words over [rho, theta, dv, dw], or one number) under the gust model `gust` (cov_rule's forms), with the
        handle's step and per-problem models.  Outputs, any but not all None: cov (B, n, 144), written at knots i0 .. i1 only; mean
        (B, n, 12); summary (B, 8): max sqrt(tr P), its knot, sqrt(tr P) at i1, max rotation deviation, the smallest clearance to a sphere
        of the handle's two tables in standard deviations, its knot, its sphere, the largest control deviation.  float64, contiguous, on
        the solver's device.  ENQUEUED on the solver's own stream and not waited for, as closed_loop_device."""
        if plan is None or plan.dim() != 3 or plan.shape[2] != KNOT:
            raise TypeError("plan must be (B, n, 18)")
        B, n = int(plan.shape[0]), int(plan.shape[1])
        i1 = n - 1 if i1 is None else int(i1)
        self._device_tensors(((plan, "plan", (B, n, KNOT)), (gains, "gains", (B, n, GAIN)), (cov, "cov", (B, n, COV)), (mean, "mean", (B, n, 12)),
                              (summary, "summary", (B, COV_SUMMARY))))
        rule = cov_rule(state_sigma, gust, wrench_held)
        if wait_current_stream:
            self._wait_current_stream(plan)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_covariance_device(self._h, C.byref(rule), vp(plan), vp(gains), C.c_int32(B), C.c_int32(n), C.c_int32(int(i0)), C.c_int32(i1),
                                              vp(cov), vp(mean), vp(summary)))

    # ---- fleet deconfliction: neighbours of every vehicle as moving spheres, and the per-problem table set from the device
    def fleet_neighbours_device(self, plan, V, K, radius, weight, range=np.inf, conflict=None, cover=False, yield_to_lower=False, summary=None,
                                nbr=None, spheres=None, counts=None, wait_current_stream=True):
        """qilqr_fleet_neighbours_device on torch tensors: plan (B, n, 18) holds plans in one world frame on one time base; rows b with equal
        b // V form a fleet.  Per vehicle the min(K, candidates) partners of its fleet with the smallest distance over the horizon, in the
        order (distance, row), and each one closer than `range` as the constant-velocity sphere {c, v, radius, weight} of
        set_batch_obstacles_device (fleet_rule's arguments).  Outputs, any but not all None: summary (B, 8); nbr (B, K, 4); spheres
        (B, K, 8); counts int32 (B).  float64, contiguous, on the solver's device.  ENQUEUED on the solver's own stream and not waited for,
        as closed_loop_device."""
        if plan is None or plan.dim() != 3 or plan.shape[2] != KNOT:
            raise TypeError("plan must be (B, n, 18)")
        import torch
        B, n, V, K = int(plan.shape[0]), int(plan.shape[1]), int(V), int(K)
        self._device_tensors(((plan, "plan", (B, n, KNOT)), (summary, "summary", (B, FLEET_SUMMARY)), (nbr, "nbr", (B, K, FLEET_NBR)),
                              (spheres, "spheres", (B, K, 8)), (counts, "counts", (B,), torch.int32)))
        rule = fleet_rule(radius, weight, range, conflict, cover, yield_to_lower)
        if wait_current_stream:
            self._wait_current_stream(plan)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_fleet_neighbours_device(self._h, C.byref(rule), vp(plan), C.c_int32(B), C.c_int32(n), C.c_int32(V), C.c_int32(K), vp(summary),
                                                    vp(nbr), vp(spheres), vp(counts)))

    def set_batch_obstacles_device(self, spheres, counts=None, dropped=None, wait_current_stream=True):
        """qilqr_set_batch_obstacles_device on torch tensors: spheres (B, K, 8) float64 and counts int32 (B) or None, as set_batch_obstacles
        takes them but on the solver's device, become the handle's per-problem table without the host; a used row with a non-finite word,
        radius <= 0 or weight < 0 is dropped (the rows kept move up) and their number goes to dropped, int32 (1), when given.  ENQUEUED on
        the solver's own stream and not waited for; clear_batch_obstacles() switches the table off again."""
        if spheres is None or spheres.dim() != 3 or spheres.shape[2] != 8:
            raise TypeError("spheres must be (B, K, 8)")
        import torch
        B, K = int(spheres.shape[0]), int(spheres.shape[1])
        self._device_tensors(((spheres, "spheres", (B, K, 8)), (counts, "counts", (B,), torch.int32), (dropped, "dropped", (1,), torch.int32)))
        if wait_current_stream:
            self._wait_current_stream(spheres)
        vp = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        _check(load().qilqr_set_batch_obstacles_device(self._h, vp(spheres), vp(counts), C.c_int32(B), C.c_int32(K), vp(dropped)))

    def profile_get(self):
        p = Profile()
        _check(load().qilqr_profile_get(self._h, C.byref(p)))
        return {f: getattr(p, f) for f, _ in Profile._fields_}

    def round_launches(self):
        """qilqr_round_launches: int32[15], the k_round launches per instantiation since the handle was created or since profile_reset();
        index 5 * (LK - 1) + j, j = 0..4 for (ROUNDS, SIX) = (1, F), (1, T), (2, F), (4, F), (4, T)"""
        counts = np.zeros(ROUND_KERNELS, dtype=np.int32)
        _check(load().qilqr_round_launches(self._h, _ip(counts)))
        return counts


class QuadrotorILQRSharded:
    """One batch over several devices from one process (qilqr_sharded_*): contiguous shards in the order of `devices`
    (an ordinal may repeat), one solver, stream and host thread per shard, results in place -- problem by problem identical
    to QuadrotorILQRBatch.solve_batch.  The one-process-per-GPU deployment (torch.distributed) is in sharding.py / bench.py."""

    def __init__(self, mass_kg, inertia, arm_length_m, torque_to_thrust_ratio_m, g_mpss, Q, R, desired, dt_s, options,
                 devices=(0,), profile=0, sync_every=2, force_general=False, single_wave_rollout=False, precision="f64",
                 streams=0, persistent=0, compaction=0, round_launch=0, rounds_per_launch=0, fuse_in_flight=0, dense_weights=0):
        lib = load()
        m, Q, R, o, dc = _create_args(self, mass_kg, inertia, arm_length_m, torque_to_thrust_ratio_m, g_mpss, Q, R, desired, options,
                                      0, profile, sync_every, force_general, single_wave_rollout, precision, streams, persistent, compaction,
                                      round_launch, rounds_per_launch, fuse_in_flight, dense_weights)
        self.devices = [int(d) for d in devices]
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        self._h = C.c_void_p()
        rc = lib.qilqr_sharded_create_sized(C.byref(m), _p(Q), _p(R), _p(self.desired), C.c_int32(len(self.desired)), C.c_double(dt_s),
                                            C.byref(o), C.byref(dc), C.c_size_t(C.sizeof(dc)), arr, C.c_int32(len(self.devices)), C.byref(self._h))
        if rc:
            self._h = None
        _check(rc)

    def close(self):
        if getattr(self, "_h", None):
            load().qilqr_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard_ranges(self, B):
        """[(begin, count)] of every shard for a batch of B (qilqr_shard_range)"""
        out = []
        for r in range(len(self.devices)):
            b0, cnt = C.c_int32(), C.c_int32()
            _check(load().qilqr_shard_range(C.c_int32(B), C.c_int32(len(self.devices)), C.c_int32(r), C.byref(b0), C.byref(cnt)))
            out.append((b0.value, cnt.value))
        return out

    def solve_batch(self, init, desired_batch=None, out=None):
        init = _d(init)
        B, n = init.shape[0], init.shape[1]
        des = None if desired_batch is None else _d(desired_batch)
        out = _batch_outputs(init, out)
        _check(load().qilqr_solve_batch_sharded(self._h, _p(init), _p(des), C.c_int32(B), C.c_int32(n), _p(out["traj"]), _p(out["cost"]),
                                                _ip(out["status"]), _ip(out["iters"]), _ip(out["n_bwd"]), _ip(out["n_fwd"])))
        return out


    def set_control_limits(self, lo, hi):
        """QuadrotorILQRBatch.set_control_limits on every shard's solver"""
        lo = _d(np.broadcast_to(np.asarray(lo, dtype=np.float64), (4,)))
        hi = _d(np.broadcast_to(np.asarray(hi, dtype=np.float64), (4,)))
        for r in range(len(self.devices)):
            _check(load().qilqr_set_control_limits(load().qilqr_sharded_solver(self._h, C.c_int32(r)), _p(lo), _p(hi)))

    def set_models(self, models):
        """QuadrotorILQRBatch.set_models for the sharded batch: each shard's solver gets its slice (qilqr_sharded_set_batch_models)"""
        arr = model_array(models)
        _check(load().qilqr_sharded_set_batch_models(self._h, C.cast(arr, C.c_void_p), C.c_int32(len(arr))), _raise_models)

    def clear_models(self):
        _check(load().qilqr_sharded_set_batch_models(self._h, None, C.c_int32(0)))

    def set_obstacles(self, spheres):
        """QuadrotorILQRBatch.set_obstacles on every shard's solver (qilqr_sharded_set_obstacles)"""
        arr = obstacle_array(spheres)
        _check(load().qilqr_sharded_set_obstacles(self._h, _p(arr), C.c_int32(len(arr))))

    def clear_obstacles(self):
        _check(load().qilqr_sharded_set_obstacles(self._h, None, C.c_int32(0)))

    def set_batch_obstacles(self, spheres, counts=None):
        """QuadrotorILQRBatch.set_batch_obstacles for the sharded batch: each shard's solver gets its rows (qilqr_sharded_set_batch_obstacles)"""
        arr, cnt = batch_obstacle_arrays(spheres, counts)
        _check(load().qilqr_sharded_set_batch_obstacles(self._h, _p(arr), _ip(cnt), C.c_int32(arr.shape[0]), C.c_int32(arr.shape[1])))

    def clear_batch_obstacles(self):
        _check(load().qilqr_sharded_set_batch_obstacles(self._h, None, None, C.c_int32(0), C.c_int32(0)))

    def set_state_weight_schedule(self, Qs):
        """QuadrotorILQRBatch.set_state_weight_schedule on every shard's solver (qilqr_sharded_set_state_weight_schedule)"""
        arr = schedule_array(Qs)
        _check(load().qilqr_sharded_set_state_weight_schedule(self._h, _p(arr), C.c_int32(len(arr))))

    def clear_state_weight_schedule(self):
        _check(load().qilqr_sharded_set_state_weight_schedule(self._h, None, C.c_int32(0)))

    def set_horizon_start(self, k0):
        """QuadrotorILQRBatch.set_horizon_start on every shard's solver (qilqr_sharded_set_horizon_start: checked once, all or none)"""
        _check(load().qilqr_sharded_set_horizon_start(self._h, C.c_int32(int(k0))))

    def clear_control_limits(self):
        for r in range(len(self.devices)):
            _check(load().qilqr_set_control_limits(load().qilqr_sharded_solver(self._h, C.c_int32(r)), None, None))

    TRANSPORTS = {"auto": 0, "rccl": 1, "peer_copy": 2}

    def set_transport(self, transport):
        """how qilqr_solve_batch_sharded_device moves the shards' rows to the root: 'auto', 'rccl' (ncclSend / ncclRecv), 'peer_copy'"""
        _check(load().qilqr_sharded_set_transport(self._h, C.c_int32(self.TRANSPORTS[transport])))
        return self.transport()

    def transport(self):
        return load().qilqr_sharded_transport(self._h).decode()

    def solve_batch_gathered(self, init, out_traj, out_cost, out_status, out_iters, out_n_bwd, out_n_fwd, desired_batch=None, root=0):
        """qilqr_solve_batch_sharded_device: host inputs, results gathered into device arrays on the device of shard `root`:
        traj (B, n, 18) float64, cost (B,) float64, the rest (B,) int32; any may be None.  An output is a raw device address
        (int: the caller vouches for its size) or a contiguous torch tensor of that dtype and shape on that device.
        Returns the exposed gather time in ms."""
        init = _d(init)
        B, n = init.shape[0], init.shape[1]
        des = None if desired_batch is None else _d(desired_batch)

        def ptr(t, dtype, shape):
            if t is None:
                return None
            if isinstance(t, int):
                return C.c_void_p(t)
            if str(t.dtype) != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device.index != self.devices[root]:
                raise ValueError(f"output tensor must be contiguous {dtype} {shape} on device {self.devices[root]}")
            return C.c_void_p(t.data_ptr())

        ms = C.c_double(0.0)
        _check(load().qilqr_solve_batch_sharded_device(
            self._h, _p(init), _p(des), C.c_int32(B), C.c_int32(n), C.c_int32(root), ptr(out_traj, "torch.float64", (B, n, 18)),
            ptr(out_cost, "torch.float64", (B,)), ptr(out_status, "torch.int32", (B,)), ptr(out_iters, "torch.int32", (B,)),
            ptr(out_n_bwd, "torch.int32", (B,)), ptr(out_n_fwd, "torch.int32", (B,)), C.byref(ms)))
        return ms.value


def gather_schedule(B, n, devices, root=0, arrays=63):
    """qilqr_gather_schedule: the transfers of qilqr_solve_batch_sharded_device for these shards, computed without touching a
    device -- list of dicts {shard, array, src_rank, dst_rank, src_off, dst_off, count}"""
    dv = np.ascontiguousarray(devices, dtype=np.int32)
    fn = load().qilqr_gather_schedule
    fn.restype = C.c_int
    args = (C.c_int32(B), C.c_int32(n), dv.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(len(dv)), C.c_int32(root), C.c_uint32(arrays))
    cnt = fn(*args, None, C.c_int32(0))
    if cnt < 0:
        raise ValueError("qilqr_gather_schedule: bad arguments")
    out = np.zeros((max(cnt, 1), 7), dtype=np.int64)
    fn(*args, out.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int32(cnt))
    keys = ("shard", "array", "src_rank", "dst_rank", "src_off", "dst_off", "count")
    return [dict(zip(keys, (int(v) for v in row))) for row in out[:cnt]]


def sharded_from_config(cfg, devices=(0,), **kw):
    return QuadrotorILQRSharded(**cfg["model"], Q=cfg["Q"], R=cfg["R"], desired=cfg["desired"], dt_s=cfg["dt"],
                                options=cfg["options"], devices=devices, **kw)


def host_array(shape, dtype=np.float64):
    """A NumPy array in pinned host memory (qilqr_host_alloc): hipMemcpy to / from it is direct DMA.  The memory is
    released when the array (and every view of it) is garbage collected."""
    import weakref
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = load().qilqr_host_alloc(C.c_size_t(max(n, 1)))
    if not p:
        raise MemoryError(load().qilqr_last_error().decode())
    buf = (C.c_char * max(n, 1)).from_address(p)
    a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    weakref.finalize(buf, load().qilqr_host_free, C.c_void_p(p))
    return a


PIN_ARITHMETIC = dict(single_wave_rollout=3)  # QILQR_PIN_ARITHMETIC of the header: one rollout kernel at every batch size (the backward pass needs no pinning since round 6)


def from_config(cfg, **kw):
    """Build a solver from a quadrotorilqr_amd.problems config dict."""
    m = cfg["model"]
    return QuadrotorILQRBatch(m["mass_kg"], m["inertia"], m["arm_length_m"], m["torque_to_thrust_ratio_m"],
                              m["g_mpss"], cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], cfg["options"], **kw)
