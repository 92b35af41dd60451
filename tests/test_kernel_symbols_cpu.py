"""The set of gfx950 kernels the library holds, by symbol name (CPU suite: hipcc -S cross-compiles without a GPU), for the product build and
for the diagnostics build (-DQILQR_DIAG), against tests/golden/kernel_symbols.json.  The host side instantiates the kernels -- k_linearize's
from a rule (route.h, lin_instantiated), the others by name in the launch helpers -- so a kernel added or lost by a change of host code
shows here, by name.  Only the names of the kernels are read, no instruction.

Every translation unit of SRCS in csrc/Makefile has its list: ilqr_capi.hip's are the golden's "product" and "diag", the five other
units' are under "units" (unit -> build -> names)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrotorilqr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
UNITS = ("shift", "closed_loop", "closed_loop_scored", "monte_carlo", "risk")  # SRCS of csrc/Makefile without ilqr_capi.hip
BUILDS = [("product", []), ("diag", ["-DQILQR_DIAG"])]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "kernel_symbols.json")) as f:
        return json.load(f)


def sources():
    out = [os.path.join(ROOT, "include", "quadrotor_ilqr.h")]
    for d, _, files in os.walk(CSRC):
        out += [os.path.join(d, f) for f in files if f.endswith((".h", ".inc", ".hip"))]
    return out


def kernel_symbols(build, defines, unit="ilqr_capi"):
    """sorted names of the .amdhsa_kernel descriptors of the device assembly of one translation unit of the build (kept between runs
    while no source is newer)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    # (the product build's assembly of ilqr_capi.hip is the file tests/test_isa_invariants.py keeps, made by the same command)
    tag = ("" if unit == "ilqr_capi" else "_" + unit) + ("" if build == "product" else "_" + build)
    asm = os.path.join(ROOT, "tests", "_device_code%s.s" % tag)
    if not os.path.exists(asm) or any(os.path.getmtime(asm) < os.path.getmtime(f) for f in sources()):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + defines +
                              ["-S", "--cuda-device-only", "-o", asm, os.path.join(CSRC, unit + ".hip")], stderr=subprocess.DEVNULL)
    with open(asm) as f:
        return sorted({line.split()[1] for line in f if line.lstrip().startswith(".amdhsa_kernel ")})


def makefile_units():
    """the translation units csrc/Makefile compiles into the library, without their suffix"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        line = next(ln for ln in f if ln.startswith("SRCS"))
    return [s[:-len(".hip")] for s in line.split(":=")[1].split()]


@pytest.mark.parametrize("build, defines", BUILDS)
def test_the_kernels_are_the_recorded_ones(golden, build, defines):
    got, want = set(kernel_symbols(build, defines)), set(golden[build])
    assert len(want) == len(golden[build]) >= 100
    assert got == want, {"built but not recorded": sorted(got - want), "recorded but not built": sorted(want - got)}


def test_every_unit_of_the_makefile_has_its_lists(golden):
    assert makefile_units() == ["ilqr_capi"] + list(UNITS)
    assert sorted(golden["units"]) == sorted(UNITS) and all(sorted(golden["units"][u]) == ["diag", "product"] for u in UNITS)


@pytest.mark.parametrize("build, defines", BUILDS)
@pytest.mark.parametrize("unit", UNITS)
def test_the_kernels_of_every_other_unit_are_the_recorded_ones(golden, unit, build, defines):
    recorded = golden["units"][unit][build]
    got, want = set(kernel_symbols(build, defines, unit)), set(recorded)
    assert len(want) == len(recorded) >= 1
    assert got == want, {"built but not recorded": sorted(got - want), "recorded but not built": sorted(want - got)}
    # no kernel of one unit is another's: a name the lists hold twice would be one kernel compiled into two units
    elsewhere = set(golden[build]).union(*(golden["units"][u][build] for u in UNITS if u != unit))
    assert not want & elsewhere, sorted(want & elsewhere)
