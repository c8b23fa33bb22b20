#!/usr/bin/env python3
"""Compare the stream operations two builds issue for the same calls, from two rocprofv3 runs
(--hip-trace --kernel-trace --output-format csv) of the same program:

    tools/stream_order_diff.py OLD_DIR NEW_DIR [--prefix r0]

Per host thread (numbered by first traced call), in issue order: every kernel launch as
(API name, kernel name, grid, stream), joined to the kernel trace by correlation id, and every
hipEventRecord / hipStreamWaitEvent / hipStreamWaitValue64 / hipMemcpy* / hipMemset* call by name.
Streams are numbered by first appearance. The CSV output carries no arguments of the event calls,
so their streams are not compared: their position among the launches (whose streams are) is.
Exit status 0 when the lists are equal, 1 with the first difference otherwise.
"""
import argparse
import csv
import os
import sys

OPS = ("hipEventRecord", "hipStreamWaitEvent", "hipStreamWaitValue64", "hipMemcpy", "hipMemset")
LAUNCH = ("hipLaunchKernel", "hipExtLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel",
          "hipLaunchCooperativeKernel")


def rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def operations(directory, prefix):
    kernels = {}
    for k in rows(os.path.join(directory, prefix + "_kernel_trace.csv")):
        kernels[k["Correlation_Id"]] = (k["Kernel_Name"], k["Grid_Size_X"], k["Grid_Size_Y"], k["Grid_Size_Z"],
                                        k["Workgroup_Size_X"], k["Stream_Id"])
    api = rows(os.path.join(directory, prefix + "_hip_api_trace.csv"))
    api.sort(key=lambda r: int(r["Start_Timestamp"]))
    threads, streams, per_thread = {}, {}, {}
    for r in api:
        name = r["Function"]
        if name in LAUNCH:
            k = kernels.get(r["Correlation_Id"])
            if k is None:
                op = (name, "?")
            else:
                op = (name,) + k[:5] + ("stream %d" % streams.setdefault(k[5], len(streams)),)
        elif name.startswith(OPS):
            op = (name,)
        else:
            continue
        t = threads.setdefault(r["Thread_Id"], len(threads))
        per_thread.setdefault(t, []).append(op)
    return per_thread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--prefix", default="r0")
    a = ap.parse_args()
    old, new = operations(a.old, a.prefix), operations(a.new, a.prefix)
    ok = sorted(old) == sorted(new)
    if not ok:
        print("threads issuing stream operations: %d vs %d" % (len(old), len(new)))
    for t in sorted(set(old) & set(new)):
        x, y = old[t], new[t]
        launches = sum(1 for op in x if len(op) > 1)
        if x == y:
            print("thread %d: %d operations (%d kernel launches) equal" % (t, len(x), launches))
            continue
        ok = False
        i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print("thread %d: %d vs %d operations, first difference at %d:" % (t, len(x), len(y), i))
        for j in range(max(0, i - 3), i + 4):
            print("  %5d  old %s\n         new %s" % (j, x[j] if j < len(x) else "-", y[j] if j < len(y) else "-"))
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
