#!/usr/bin/env python3
"""Diagnostic: static instruction histogram of the sixteen-lane rollout step's loop in one kernel of the device assembly
(hipcc -O3 --offload-arch=gfx950 -S --cuda-device-only ilqr_capi.hip; tests/_device_code.s is such a file).

The loops are found from the assembly alone: a backward branch whose span (from its target label to the branch) holds the step's
broadcast-multiply-adds (v_fmac_f64_dpp: 35 per step) and no smaller such span inside it.  Counted is what stands between the label and
the branch in layout order -- blocks the compiler moved behind the loop (the rare sides) are not in it, blocks it left inside are.
Static counts, not measurements.
usage: python3 profiles/microbench/step_histogram.py file.s [mangled-name-prefix = _ZN5qilqr7k_roundILi3ELi4ELb0E]"""
import re
import sys


def classify(op):
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc")):
        return "branch"
    if op in ("v_mov_b32_dpp", "v_mov_b64_dpp"):
        return op
    if op.endswith("_dpp") and "f64" in op:
        return "fp64 arithmetic"
    if re.match(r"v_(fma|fmac|mul|add|sub|min|max|rcp|div_\w+|cmp_\w+|cmpx_\w+|cndmask|sqrt|rsq|ldexp|frexp\w*|trig\w*)_\w*f64", op):
        return "fp64 compare" if op.startswith("v_cmp") else "fp64 arithmetic"
    if op == "v_cndmask_b32_e32" or op.startswith("v_cndmask"):
        return "v_cndmask"
    if op in ("v_mov_b64_e32", "v_mov_b32_e32", "v_accvgpr_read_b32", "v_accvgpr_write_b32"):
        return "vector moves"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "vector memory"
    if op.startswith("s_"):
        return "other scalar"
    return "other vector"


def main():
    path = sys.argv[1]
    prefix = sys.argv[2] if len(sys.argv) > 2 else "_ZN5qilqr7k_roundILi3ELi4ELb0E"
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(":")[0].startswith(prefix) and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("\t.size\t" + prefix))
    body = lines[start:end]
    label_at = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    ins = [(i, l.split()[0], l) for i, l in enumerate(body) if l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;")]
    spans = []
    for i, op, l in ins:
        if op.startswith(("s_cbranch", "s_branch")):
            t = label_at.get(l.split()[1])
            if t is not None and t < i:
                n = sum(1 for j, o, _ in ins if t <= j <= i and o == "v_fmac_f64_dpp")
                if n >= 30:
                    spans.append((t, i, n))
    inner = [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    print(f"{prefix}: {len(inner)} step loops")
    for t, i, n in inner:
        hist = {}
        for j, op, _ in ins:
            if t <= j <= i:
                hist[classify(op)] = hist.get(classify(op), 0) + 1
        blocks = sum(1 for lab, at in label_at.items() if t <= at <= i)
        total = sum(hist.values())
        print(f"  lines {start + t + 1}..{start + i + 1}: {total} instructions, {blocks} basic blocks, {n} v_fmac_f64_dpp")
        for k in sorted(hist, key=lambda k: -hist[k]):
            print(f"    {k:18s} {hist[k]:4d}")


if __name__ == "__main__":
    main()
