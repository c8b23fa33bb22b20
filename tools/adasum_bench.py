#!/usr/bin/env python3
"""What the Adasum pair (tips_adasum_pair) costs, by tools/scaled_bench.py's method:
rotating buffer sets (no launch finds its operands in the Infinity Cache), HIP events on the launch
stream, a warm-up, and in one process, alternated repetition by repetition:

  (a) pair        tips_adasum_pair: dots + coef + combine, 5 passes over a buffer's bytes
  (b) bucket_sum  tips_bucket_sum on the same buffers: 3 passes - this process's streaming yardstick

Shapes: 2 x 256 MiB f32 as one segment; config 5's 214 gradient counts in f32 as one list; 2 x 256
MiB bf16 as one segment. share = (5 passes of the buffer's bytes at 8 TB/s) / the pair's median, and
the same with 3 passes for the sum. The events time the three launches together; the dots and the
combine each alone come from a kernel trace of `--legs pair` (the per-kernel durations), and their
bounds are 2 and 3 passes. No ratio is fixed in advance: the records say what was measured.
Prints one JSON line per shape; --out appends them to a file (profiles/adasum/).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROTATE_BYTES = 1536 << 20  # one rotation through the sets moves far more than the Infinity Cache holds
PEAK = 8e12


def shapes():
    from bench import resnet50_grad_sizes
    n32 = (256 << 20) // 4
    return [("1seg_256MiB_f32", "f32", [n32]), ("config5_214_f32", "f32", [int(c) for c in resnet50_grad_sizes()]),
            ("1seg_256MiB_bf16", "bf16", [(256 << 20) // 2])]


def measure(name, dt, counts, steps, warmup, reps, legs_wanted):
    import torch
    from tips_amd import _lib
    code, tdt, es = (_lib.FLOAT32, torch.float32, 4) if dt == "f32" else (_lib.BFLOAT16, torch.bfloat16, 2)
    n = sum(counts)
    need = _lib.lib().tips_adasum_workspace(n, len(counts))
    nsets = max(3, -(-ROTATE_BYTES // (3 * n * es)))
    g = torch.Generator(device="cuda")
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    cp = _lib.i64_array(counts)
    sets = []
    for k in range(nsets):
        ab = []
        for j in range(2):
            g.manual_seed(10 * k + j + 1)
            ab.append(torch.empty(n, dtype=torch.float32, device="cuda").normal_(generator=g).to(tdt))
        sets.append((ab[0], ab[1], torch.empty(n, dtype=tdt, device="cuda"),
                     torch.empty(need, dtype=torch.uint8, device="cuda")))

    def pair(i):
        a, b, out, ws = sets[i % nsets]
        _lib.call("tips_adasum_pair", out.data_ptr(), a.data_ptr(), b.data_ptr(), cp[0], len(counts), code, ws.data_ptr(),
                  need, sp)

    def bucket_sum(i):
        a, b, out, _ = sets[i % nsets]
        _lib.call("tips_bucket_sum", out.data_ptr(), a.data_ptr(), b.data_ptr(), n, code, sp)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(steps):
            fn(i)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3  # us per step

    legs = [(k, f) for k, f in (("pair", pair), ("bucket_sum", bucket_sum)) if k in legs_wanted]
    for _, fn in legs:
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    us = {k: [] for k, _ in legs}
    for _ in range(reps):  # alternated: drift over the run lands on every leg alike
        for k, fn in legs:
            us[k].append(timed(fn))
    rec = {"shape": name, "dtype": dt, "segments": len(counts), "elements": n, "bytes_per_buffer": n * es, "steps": steps,
           "warmup": warmup, "reps": reps, "rotating_sets": nsets, "device": torch.cuda.get_device_name(0)}
    passes = {"pair": 5, "bucket_sum": 3}
    for k in us:
        v = sorted(us[k])
        med = v[len(v) // 2]
        rec[k] = {"us_median": round(med, 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2),
                  "bound_us_at_8TBps": round(passes[k] * n * es / PEAK * 1e6, 2),
                  "share_of_bound": round(passes[k] * n * es / PEAK * 1e6 / med, 4)}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="pair,bucket_sum")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    for name, dt, counts in shapes():
        if args.shape and args.shape != name:
            continue
        rec = measure(name, dt, counts, args.steps, args.warmup, args.reps, args.legs.split(","))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
