"""The cases of tests/closed_loop_cases.py are the kernels of the closed-loop flight family: closed_loop.hip and closed_loop_scored.hip
cross-compiled to device assembly (the command and the keep-while-fresh files of tests/test_kernel_symbols_cpu.py, one per unit) hold 16 + 48
kernels, every one named by exactly one case and every case naming one that was built.  The template arguments are read from the mangled
names alone; no instruction is read.  And the S of each form takes that form: closed_loop_shared_form (closed_loop_kernels.h) compiled for
the host in tests/host_closed_loop_harness.cpp."""
import subprocess

import pytest

from tests import closed_loop_cases as cc
from tests.test_closed_loop_cpu import build_harness
from tests.test_kernel_symbols_cpu import kernel_symbols


@pytest.fixture(scope="module")
def built():
    """the kernels of the two units, product build"""
    return {unit: kernel_symbols("product", [], unit) for unit in ("closed_loop", "closed_loop_scored")}


def test_the_cases_are_the_kernels_one_to_one(built):
    assert len(built["closed_loop"]) == 16 and len(built["closed_loop_scored"]) == 48
    kernels = set(built["closed_loop"]) | set(built["closed_loop_scored"])
    assert len(cc.CASES) == len(set(cc.CASES)) == 64 and len({cc.name(c) for c in cc.CASES}) == 64
    named = [cc.kernel_name(c) for c in cc.CASES]
    assert len(set(named)) == 64  # no kernel is named by two cases
    assert set(named) == kernels, {"built and named by no case": sorted(kernels - set(named)), "named and not built": sorted(set(named) - kernels)}
    # the unit of a case: without a wrench and a score the call is k_closed_loop's
    for c in cc.CASES:
        assert cc.kernel_name(c) in built["closed_loop" if not (c.wrench or c.score) else "closed_loop_scored"], cc.name(c)


def test_the_template_arguments_read_from_a_symbol_are_its_cases(built):
    """the other way round, from the built symbols alone: each spells the arguments of one case, and no two the same"""
    read = {k: cc.case_of(k) for unit in built.values() for k in unit}
    assert all(c is not None for c in read.values()), [k for k, c in read.items() if c is None]
    assert sorted(read.values()) == sorted(cc.CASES)
    assert all(cc.kernel_name(c) == k for k, c in read.items())
    assert cc.case_of("_ZN5qilqr9k_rolloutIfLi0EJEEEvNS_11ModelConstsIT_EENS_10BatchStateEiiiDpT1_") is None  # (a kernel of another family)


def test_the_diagnostics_build_holds_the_same_family():
    for unit in ("closed_loop", "closed_loop_scored"):
        assert kernel_symbols("diag", ["-DQILQR_DIAG"], unit) == kernel_symbols("product", [], unit)


def test_the_cases_cover_every_combination_the_issue_names():
    both = [c for c in cc.CASES if c.limits and c.models]
    assert sum(1 for c in both if not (c.wrench or c.score)) == 4 and sum(1 for c in both if c.wrench or c.score) == 12
    assert len({cc.group(c) for c in cc.CASES}) == 16 and all(sum(1 for c in cc.CASES if cc.group(c) == g) == 4 for g in {cc.group(c) for c in cc.CASES})
    assert any(c.shared and c.models and c.score and not c.wrench for c in cc.CASES) and any(c.shared and c.models and c.wrench and not c.score for c in cc.CASES)


def test_the_samples_of_each_form_take_that_form():
    exe = build_harness(["-O2"], "host_closed_loop_harness")
    ask = [1, cc.S_FLAT, 62, cc.S_SHARED, 64, 65, 70, 125, 126, 128]
    said = subprocess.run([exe, "form"] + [str(S) for S in ask], check=True, capture_output=True, text=True).stdout.split()
    assert dict(zip(ask, said)) == {1: "flattened", 5: "flattened", 62: "flattened", 63: "shared", 64: "shared", 65: "flattened", 70: "flattened",
                                    125: "flattened", 126: "shared", 128: "shared"}
    assert all(cc.samples(c) == (cc.S_SHARED if c.shared else cc.S_FLAT) for c in cc.CASES) and (cc.S_SHARED, cc.S_FLAT) == (63, 5)
