"""The per-problem models extension (qilqr_set_batch_models) on the CPU: the record builder (host_model.h, make_model_table) and the
device math read through the per-problem accessor (batch_models.h, problem_model), compiled with g++ by tests/host_models_harness.cpp,
against make_model_consts and the oracle; and the gfx950 code of the extension's kernel instantiations (hipcc -S): present, no scratch
(beyond what the Runge-Kutta linearisation spills with one shared model already)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as orc
from quadrotorilqr_amd import capi, problems as pb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "quadrotorilqr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
DT = 0.07


def random_models(count, seed):
    """as tests/test_gpu_parity.py::randomised_cfg draws one: mass 0.5..3 kg, random SPD inertia, arm, torque ratio, g"""
    r = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        A = r.uniform(-0.3, 0.3, (3, 3))
        out.append(dict(mass_kg=r.uniform(0.5, 3.0), inertia=A @ A.T + np.diag(r.uniform(0.5, 2.0, 3)),
                        arm_length_m=r.uniform(0.2, 1.2), torque_to_thrust_ratio_m=r.uniform(0.05, 0.5), g_mpss=r.uniform(3.0, 12.0)))
    return out


@pytest.fixture(scope="module")
def hm():
    d = tempfile.mkdtemp(prefix="host_models_harness_")
    so = os.path.join(d, "libhost_models_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_models_harness.cpp"), "-lm"])
    lib = C.CDLL(so)
    lib.hm_model_table.restype = C.c_long
    lib.hm_model_table.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.hm_model_consts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.hm_problem_step.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int] + [C.c_void_p] * 5
    return lib


def V(a):
    return a.ctypes.data_as(C.c_void_p)


def table(hm, models, Q=pb.Q_DEMO, R=pb.R_DEMO, dt=DT):
    arr = capi.model_array(models)
    tab = np.zeros((len(arr), hm.hm_words()))
    bad = hm.hm_model_table(C.cast(arr, C.c_void_p), len(arr), V(np.ascontiguousarray(Q, dtype=float)),
                            V(np.ascontiguousarray(R, dtype=float)), dt, V(tab))
    return bad, tab


def consts(hm, model, Q=pb.Q_DEMO, R=pb.R_DEMO, dt=DT):
    """make_model_consts of one model, as the flat ModelConsts<double>: dt, mass, g, inertia, inertia_inv, arms, Bu, Q, R"""
    buf = np.zeros(hm.hm_consts_size() // 8)
    arr = capi.model_array([model])
    assert hm.hm_model_consts(C.cast(arr, C.c_void_p), V(np.ascontiguousarray(Q, dtype=float)), V(np.ascontiguousarray(R, dtype=float)),
                              dt, V(buf)) == 0
    return buf


def test_record_builder_gives_the_bits_of_make_model_consts(hm):
    models = random_models(24, seed=5) + [pb.MODEL_D, pb.MODEL_A]
    bad, tab = table(hm, models)
    assert bad == -1 and tab.shape == (26, 48)
    for b, m in enumerate(models):
        c = consts(hm, m)
        mass, g, inertia, inertia_inv, arms, Bu = c[1], c[2], c[3:12], c[12:21], c[21:33], c[33:81].reshape(12, 4)
        rec = tab[b]
        want = np.concatenate([[mass, g], inertia, inertia_inv, arms, Bu[8:].reshape(16)])
        assert want.tobytes() == rec.tobytes(), b  # bit for bit
        assert not Bu[:8].any()  # (the rows a record leaves out are zero for every model)
    assert len({tab[b].tobytes() for b in range(len(models))}) == len(models)


def test_record_builder_reports_the_first_bad_inertia(hm):
    models = random_models(12, seed=6)
    models[7] = dict(models[7], inertia=np.diag([1.0, -1.0, 1.0]))
    asym = np.eye(3)
    asym[0, 1] = 0.2
    models[10] = dict(models[10], inertia=asym)
    assert table(hm, models)[0] == 7
    assert table(hm, models[8:])[0] == 2
    assert table(hm, models[:7])[0] == -1


def test_python_model_array_forms_agree():
    models = random_models(5, seed=8)
    cols = {k: np.array([m[k] for m in models]) for k in capi.MODEL_FIELDS}
    a, b = capi.model_array(models), capi.model_array(cols)
    assert bytes(a) == bytes(b)
    # scalars (and one 3 x 3 inertia) broadcast over the batch
    c = capi.model_array(dict(pb.MODEL_D, mass_kg=np.array([1.0, 2.0, 3.0])))
    assert len(c) == 3 and [m.mass_kg for m in c] == [1.0, 2.0, 3.0] and all(m.g_mpss == 9.81 and m.inertia[4] == 1.0 for m in c)
    with pytest.raises(TypeError):
        capi.model_array(dict(pb.MODEL_D, mass_kg=np.ones(3), g_mpss=np.ones(4)))


@pytest.mark.parametrize("integ", [0, 1])
def test_device_math_through_the_accessor_matches_the_oracle_per_model(hm, integ):
    """One step of the device code and the Jacobians the backward kernel reads, for problem b of a table of twelve distinct models,
    against the oracle's step with that problem's own model."""
    models = random_models(12, seed=11 + integ)
    bad, tab = table(hm, models)
    assert bad == -1
    shared = consts(hm, pb.MODEL_D)  # the handle's own model: what the accessor must NOT use
    r = np.random.default_rng(3 + integ)
    ju_seen = []
    for b, m in enumerate(models):
        mp = orc.model_params(**m)
        for _ in range(3):
            x = np.concatenate([r.uniform(-2, 2, 3), orc.se3_exp(np.concatenate([np.zeros(3), r.uniform(-1.2, 1.2, 3)]))[3:],
                                r.uniform(-2, 2, 6)])
            u = r.uniform(0.0, 8.0, 4)
            xn_ref, Jx_ref, Ju_ref = orc.discrete_step(mp, integ, x, u, DT, diffs=True)
            xn, Jx, Ju = np.zeros(13), np.zeros((12, 12)), np.zeros((12, 4))
            hm.hm_problem_step(V(shared), V(tab), b, integ, V(x), V(u), V(xn), V(Jx), V(Ju))
            np.testing.assert_allclose(xn, xn_ref, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(Jx, Jx_ref, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(Ju, Ju_ref, rtol=1e-12, atol=1e-12)
        ju_seen.append(Ju.tobytes())
    assert len(set(ju_seen)) == len(models)


# ------------------------------------------------------------------ the gfx950 code of the extension's instantiations
@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="batch_models_isa_")
    asm = os.path.join(d, "device.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                           "--cuda-device-only", "-o", asm, os.path.join(CSRC, "ilqr_capi.hip")], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        out[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
    return out


def test_the_instantiations_of_the_extension_exist_and_use_no_scratch(kernels):
    ext = {name: scratch for name, scratch in kernels.items() if "11BatchModels" in name}
    lin = [k for k in ext if "k_linearize" in k]
    rol = [k for k in ext if "k_rollout" in k]
    bwd = [k for k in ext if "k_backward_models" in k]
    assert len(lin) == 7, lin    # Euler: record kinds 0..3 (3: diagonal Q); Runge-Kutta: 0..2
    assert len(rol) == 4, rol    # either integrator, with and without ControlLimits
    assert sum("ControlLimits" in k for k in rol) == 2
    assert len(bwd) == 3, bwd    # symmetric, general, symmetric box form
    assert sum("ControlLimits" in k for k in bwd) == 1
    assert len(ext) == 14, sorted(ext)
    for name, scratch in ext.items():
        m = re.match(r"_ZN5qilqr11k_linearizeIdLi(\d)ELi1ELb0EJ", name)
        if m:
            # The Runge-Kutta dynamics half spills its 12 x 16 M in the shared-model kernel already (k_linearize<double, LK, 1, false>):
            # the per-problem form may not spill more than a record's worth beyond it
            base = [v for k, v in kernels.items() if k.startswith(f"_ZN5qilqr11k_linearizeIdLi{m.group(1)}ELi1ELb0EJEEEv")]
            assert len(base) == 1 and base[0] > 0
            assert scratch <= base[0] + 8 * 48, (name, scratch, base[0])
        else:
            assert scratch == 0, (name, scratch)
