#!/usr/bin/env python3
"""What the scale costs inside the sum kernels (Scaled allreduce), by bench.py's config-2
method: float32, 4 rotating buffer sets (no launch finds its operands in the Infinity Cache), HIP
events on the launch stream, a warm-up. In one process, alternated repetition by repetition:

  (a) the plain launch          tips_bucket_sum / tips_multi_sum        - the yardstick
  (b) the scaled launch         tips_bucket_sum_scaled / tips_multi_sum_scaled (1/3, 0.7)
  (c) today's workaround        (a) followed by an in-place tips_scale of the result

for the 2-input sum (2 x 256 MiB) and the 8-input fold (8 x 32 MiB). The expectation: (b) within
(a)'s own spread over the repetitions - the kernels are memory-bound and the traffic is the same -
and (c) near 5/3 of (a) for the 2-input sum (3 + 2 buffer passes instead of 3).

Prints one JSON line per shape; --out appends them to a file (profiles/).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROTATING_SETS = 4
PRE, POST = 1.0 / 3.0, 0.7


def measure(nsrc, mib, steps, warmup, reps):
    import torch
    from tips_amd import _lib
    F32 = _lib.FLOAT32
    n = mib * (1 << 20) // 4
    g = torch.Generator(device="cuda")
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    sets = []
    for k in range(ROTATING_SETS):
        srcs = []
        for j in range(nsrc):
            g.manual_seed(100 * k + j + 1)
            srcs.append(torch.empty(n, dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=g))
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        pp = _lib.ptr_array([s.data_ptr() for s in srcs])
        sets.append((srcs, out, pp))

    def plain(i):
        srcs, out, pp = sets[i % ROTATING_SETS]
        if nsrc == 2:
            _lib.call("tips_bucket_sum", out.data_ptr(), srcs[0].data_ptr(), srcs[1].data_ptr(), n, F32, sp)
        else:
            _lib.call("tips_multi_sum", out.data_ptr(), pp[0], nsrc, n, F32, sp)

    def scaled(i):
        srcs, out, pp = sets[i % ROTATING_SETS]
        if nsrc == 2:
            _lib.call("tips_bucket_sum_scaled", out.data_ptr(), srcs[0].data_ptr(), srcs[1].data_ptr(), n, F32, PRE, POST, sp)
        else:
            _lib.call("tips_multi_sum_scaled", out.data_ptr(), pp[0], nsrc, n, F32, PRE, POST, sp)

    def workaround(i):
        plain(i)
        out = sets[i % ROTATING_SETS][1]
        _lib.call("tips_scale", out.data_ptr(), out.data_ptr(), n, F32, PRE * POST, sp)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(steps):
            fn(i)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3  # us per step

    legs = [("plain", plain), ("scaled", scaled), ("plain_then_scale", workaround)]
    for _, fn in legs:
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(reps):  # alternated: drift over the run lands on every leg alike
        for name, fn in legs:
            us[name].append(timed(fn))
    rec = {"shape": "%d x %d MiB f32" % (nsrc, mib), "steps": steps, "warmup": warmup, "reps": reps,
           "rotating_sets": ROTATING_SETS, "factors": [PRE, POST], "device": torch.cuda.get_device_name(0)}
    for name in us:
        v = sorted(us[name])
        rec[name] = {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2),
                     "us_all": [round(x, 2) for x in us[name]]}
    a, b, c = rec["plain"], rec["scaled"], rec["plain_then_scale"]
    rec["scaled_over_plain"] = round(b["us_median"] / a["us_median"], 4)
    rec["workaround_over_plain"] = round(c["us_median"] / a["us_median"], 4)
    rec["scaled_within_plain_spread"] = bool(a["us_min"] <= b["us_median"] <= a["us_max"])
    rec["plain_GBps"] = round((nsrc + 1) * n * 4 / (a["us_median"] * 1e-6) / 1e9, 1)
    rec["scaled_GBps"] = round((nsrc + 1) * n * 4 / (b["us_median"] * 1e-6) / 1e9, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tips_amd
    torch.cuda.set_device(0)
    tips_amd.init()
    for nsrc, mib in ((2, 256), (8, 32)):
        rec = measure(nsrc, mib, args.steps, args.warmup, args.reps)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
