"""The kernels that contain the sixteen-lane rollout step (rollout16_kernel.h, r16_wave_X) keep it in registers (CPU suite: hipcc -S
cross-compiles without a GPU; the assembly is the one tests/test_isa_invariants.py builds, whichever of the two runs first).

r16_publish_stores announces a chunk of knots behind `s_waitcnt vmcnt(2)`: right only while a step issues exactly its two vector-memory
stores, so a register spilled inside the step loop would be a wrong result, not only a slower one.  Issuing the step's independent
broadcast-multiply-add chains side by side (r16::WaveExt) keeps more operands live at once, hence this check of the kernel descriptors:
no spilled vector register and no scratch memory in k_rollout16, k_backward_rollout and k_round -- but for the two k_round instantiations
with the six-wavefront backward pass and the largest record, whose backward phase spilled before the chains were grouped (46 and 4
registers at commit f88abe3): those may not spill MORE."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrotorilqr_amd", "csrc")
ASM = os.path.join(ROOT, "tests", "_device_code.s")
HIPCC = "/opt/rocm/bin/hipcc"

# (vgpr_spill_count, private_segment_fixed_size) of the kernels that spilled at commit f88abe3: k_round<1, 4, true>, k_round<1, 1, true>
BEFORE = {"_ZN5qilqr7k_roundILi1ELi4ELb1EEE": (46, 80), "_ZN5qilqr7k_roundILi1ELi1ELb1EEE": (4, 32)}


@pytest.fixture(scope="module")
def descriptors():
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc", ".hip"))] + [os.path.join(ROOT, "include", "quadrotor_ilqr.h")]
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    if not os.path.exists(ASM) or any(os.path.getmtime(ASM) < os.path.getmtime(f) for f in srcs):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                               "--cuda-device-only", "-o", ASM, os.path.join(CSRC, "ilqr_capi.hip")], stderr=subprocess.DEVNULL)
    text = open(ASM).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, entry).group(1)) for k in ("vgpr_spill_count", "private_segment_fixed_size"))
    return out


def test_the_kernels_that_contain_the_rollout_step_keep_it_in_registers(descriptors):
    with_step = {n: v for n, v in descriptors.items() if re.match(r"_ZN5qilqr(11k_rollout16|18k_backward_rollout|7k_round)I", n)}
    # k_rollout16 and k_backward_rollout for both storage types, k_round<LK = 1..3, rounds, six-wavefront backward pass>
    assert len(with_step) == 2 + 2 + 15, sorted(with_step)
    for name, (spills, scratch) in with_step.items():
        before = [v for k, v in BEFORE.items() if name.startswith(k)]
        allowed = before[0] if before else (0, 0)
        assert spills <= allowed[0] and scratch <= allowed[1], (name, spills, scratch, allowed)
