"""The set of gfx950 kernels the library holds, by symbol name (CPU suite: hipcc -S cross-compiles without a GPU), for the product build and
for the diagnostics build (-DQILQR_DIAG), against tests/golden/kernel_symbols.json.  The host side instantiates the kernels -- k_linearize's
from a rule (route.h, lin_instantiated), the others by name in the launch helpers -- so a kernel added or lost by a change of host code
shows here, by name.  Only the names of the kernels are read, no instruction."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrotorilqr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "kernel_symbols.json")) as f:
        return json.load(f)


def sources():
    out = [os.path.join(ROOT, "include", "quadrotor_ilqr.h")]
    for d, _, files in os.walk(CSRC):
        out += [os.path.join(d, f) for f in files if f.endswith((".h", ".inc", ".hip"))]
    return out


def kernel_symbols(build, defines):
    """sorted names of the .amdhsa_kernel descriptors of the build's device assembly (kept between runs while no source is newer)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    # (the product build's assembly is the file tests/test_isa_invariants.py keeps, made by the same command)
    asm = os.path.join(ROOT, "tests", "_device_code.s" if build == "product" else "_device_code_%s.s" % build)
    if not os.path.exists(asm) or any(os.path.getmtime(asm) < os.path.getmtime(f) for f in sources()):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + defines +
                              ["-S", "--cuda-device-only", "-o", asm, os.path.join(CSRC, "ilqr_capi.hip")], stderr=subprocess.DEVNULL)
    with open(asm) as f:
        return sorted({line.split()[1] for line in f if line.lstrip().startswith(".amdhsa_kernel ")})


@pytest.mark.parametrize("build, defines", [("product", []), ("diag", ["-DQILQR_DIAG"])])
def test_the_kernels_are_the_recorded_ones(golden, build, defines):
    got, want = set(kernel_symbols(build, defines)), set(golden[build])
    assert len(want) == len(golden[build]) >= 100
    assert got == want, {"built but not recorded": sorted(got - want), "recorded but not built": sorted(want - got)}
