#!/usr/bin/env python3
"""What MAX / MIN cost against the sum in the same launches (MAX and MIN), by
tools/scaled_bench.py's method: 4 rotating buffer sets (no launch finds its operands in the Infinity
Cache), HIP events on the launch stream, a warm-up. In one process, alternated repetition by
repetition:

  (a) the plain launch   tips_bucket_sum / tips_multi_sum          - the yardstick, this run's own
  (b) MAX                tips_bucket_reduce / tips_multi_reduce (TIPS_OP_MAX)
  (c) MIN                the same with TIPS_OP_MIN

for the 2-input launch (2 x 256 MiB f32) and the 8-input fold (8 x 32 MiB, f32 and bf16). The
expectation: a tie - the kernels are memory-bound and MAX / MIN move exactly the sum's bytes; for
bf16 the sum widens and rounds where the compare only widens. Accepted: (b) and (c) within 2 % of
(a)'s median (in-process alternated A/Bs here resolve about 1 %).

Each shape runs in a child process of its own under a time limit (--shape runs one shape in this
process). Prints one JSON line per shape; --out appends them to a file (profiles/).
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROTATING_SETS = 4
SHAPES = {"sum2_f32": (2, 256, "f32"), "fold8_f32": (8, 32, "f32"), "fold8_bf16": (8, 32, "bf16")}
ACCEPT = 1.02


def measure(nsrc, mib, dt, steps, warmup, reps):
    import torch
    from tips_amd import _lib
    code, tdt, es = (_lib.FLOAT32, torch.float32, 4) if dt == "f32" else (_lib.BFLOAT16, torch.bfloat16, 2)
    n = mib * (1 << 20) // es
    g = torch.Generator(device="cuda")
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    sets = []
    for k in range(ROTATING_SETS):
        srcs = []
        for j in range(nsrc):
            g.manual_seed(100 * k + j + 1)
            srcs.append(torch.empty(n, dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=g).to(tdt))
        out = torch.empty(n, dtype=tdt, device="cuda")
        pp = _lib.ptr_array([s.data_ptr() for s in srcs])
        sets.append((srcs, out, pp))

    def plain(i):
        srcs, out, pp = sets[i % ROTATING_SETS]
        if nsrc == 2:
            _lib.call("tips_bucket_sum", out.data_ptr(), srcs[0].data_ptr(), srcs[1].data_ptr(), n, code, sp)
        else:
            _lib.call("tips_multi_sum", out.data_ptr(), pp[0], nsrc, n, code, sp)

    def reduce_with(op):
        def fn(i):
            srcs, out, pp = sets[i % ROTATING_SETS]
            if nsrc == 2:
                _lib.call("tips_bucket_reduce", out.data_ptr(), srcs[0].data_ptr(), srcs[1].data_ptr(), n, code, op, sp)
            else:
                _lib.call("tips_multi_reduce", out.data_ptr(), pp[0], nsrc, n, code, op, sp)
        return fn

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(steps):
            fn(i)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3  # us per step

    legs = [("plain", plain), ("max", reduce_with(_lib.OP_MAX)), ("min", reduce_with(_lib.OP_MIN))]
    for _, fn in legs:
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(reps):  # alternated: drift over the run lands on every leg alike
        for name, fn in legs:
            us[name].append(timed(fn))
    rec = {"shape": "%d x %d MiB %s" % (nsrc, mib, dt), "steps": steps, "warmup": warmup, "reps": reps,
           "rotating_sets": ROTATING_SETS, "device": torch.cuda.get_device_name(0)}
    for name in us:
        v = sorted(us[name])
        rec[name] = {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2),
                     "us_all": [round(x, 2) for x in us[name]]}
    a = rec["plain"]["us_median"]
    rec["max_over_plain"] = round(rec["max"]["us_median"] / a, 4)
    rec["min_over_plain"] = round(rec["min"]["us_median"] / a, 4)
    rec["within_2_percent"] = bool(rec["max_over_plain"] <= ACCEPT and rec["min_over_plain"] <= ACCEPT)
    rec["plain_GBps"] = round((nsrc + 1) * n * es / (a * 1e-6) / 1e9, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help="one shape, in this process")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per shape (child processes)")
    args = ap.parse_args()
    if args.shape is None:
        for shape in SHAPES:  # a fresh process per shape, each under its own time limit; the first failure ends the run
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--steps", str(args.steps), "--warmup",
                   str(args.warmup), "--reps", str(args.reps)] + (["--out", args.out] if args.out else [])
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
            if rc != 0:
                sys.exit("shape %s exited %d" % (shape, rc))
        return
    import torch
    import tips_amd
    torch.cuda.set_device(0)
    tips_amd.init()
    rec = measure(*SHAPES[args.shape], args.steps, args.warmup, args.reps)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
