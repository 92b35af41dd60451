#!/usr/bin/env python3
"""Diagnostic: the kernels of the two fleet calls, per case, from the kernel-trace CSV of
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 profiles/microbench/fleet.py trace=1`: that run enqueues 20 pairs of
the calls at B = V = 1024 and then 20 at 16 fleets of 64, so dispatches 1..20 of a kernel are the first case and 21..40 the second (the
first of each case is left out: code object load).  usage: python3 profiles/microbench/fleet_trace_split.py DIR/.../*_kernel_trace.csv"""
import csv
import statistics as st
import sys

KERNELS = ("k_fleet_fit", "k_fleet_pairs", "k_fleet_select", "k_bob_set")
CASES = (("B = V = 1024", 1, 20), ("16 fleets of 64", 21, 40))


def main():
    by = {}
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    print("kernel; dispatches; per case the median us (min - max) over its dispatches 2..20")
    for k in KERNELS:
        d = sorted(by.get(k, []))
        out = [k, str(len(d))]
        for tag, lo, hi in CASES:
            us = [(e - s) / 1e3 for s, e in d[lo:hi]]
            if us:
                out.append("%s: %.1f (%.1f - %.1f)" % (tag, st.median(us), min(us), max(us)))
        print("; ".join(out))
    fit, bob = sorted(by.get("k_fleet_fit", [])), sorted(by.get("k_bob_set", []))
    for tag, lo, hi in CASES:
        span = [(bob[i][1] - fit[i][0]) / 1e3 for i in range(lo, min(hi, len(fit), len(bob)))]
        if span:
            print("%s: from the fit's start to the setter's end, median %.1f us" % (tag, st.median(span)))


if __name__ == "__main__":
    main()
