#!/usr/bin/env python3
"""What the reduce-scatter's fold kernel costs at one rank, by tools/mxfp8_bench.py's
method: rotating buffer sets (no launch finds its operands in the Infinity Cache), HIP events on the
launch stream, a warm-up, medians over alternated repetitions, in one process:

  fold_segs   tips_reducescatter_fold at nsrc = 8, own_pos = 0: 7 staged regions and the own slices
              read, the outputs written - 9 x the payload bytes
  multi_sum   tips_multi_sum of 8 contiguous buffers of the same element count into a ninth: the
              existing fold kernel, the yardstick

Shapes: (a) one 32 MiB f32 segment; (b) slice 0 of 8 of config 5's 214 gradients (each taken as a
[count] tensor, so slice 0 holds ceil(count / 8) elements), own slices and outputs each on a 256-B
boundary as separate allocations are; (c) the same in bf16. share = the bytes-only bound at 8 TB/s /
the median; ratio = multi_sum's median / fold_segs' median. No ratio is fixed in advance: the records
say what was measured. The collective itself (the exchange over xGMI) cannot be measured on one GPU.
Prints one JSON line per shape; --out appends them to a file (profiles/reducescatter/).
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROTATE_BYTES = 1536 << 20
PEAK = 8e12
NSRC = 8


def shapes():
    from bench import resnet50_grad_sizes
    from tips_amd import _lib
    grads = [int(c) for c in resnet50_grad_sizes()]
    slice0 = [-(-c // NSRC) for c in grads]
    return [("1x32MiB_f32", [(32 << 20) // 4], _lib.FLOAT32), ("config5_214_slice0of8_f32", slice0, _lib.FLOAT32),
            ("config5_214_slice0of8_bf16", slice0, _lib.BFLOAT16)]


def measure(name, counts, code, steps, warmup, reps):
    import torch
    import tips_amd
    from tips_amd import _lib
    tips_amd.init()
    es = 2 if code == _lib.BFLOAT16 else 4
    tdt = torch.bfloat16 if code == _lib.BFLOAT16 else torch.float32
    n = sum(counts)
    ones = [1] * len(counts)
    cp, ep = _lib.i64_array(counts), _lib.i64_array(ones)
    offs = (ctypes.c_int64 * len(counts))()
    region = _lib.call("tips_reducescatter_layout", cp[0], ep[0], len(counts), code, 1, 0, offs)  # (the slices as given)
    offs = [int(o) for o in offs]
    relems = -(-region // 256) * 256 // es
    per_set = (NSRC + 1) * relems * es
    nsets = max(3, -(-ROTATE_BYTES // per_set))
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(18)

    def filled(elems):
        return torch.empty(elems, dtype=torch.float32, device="cuda").normal_(generator=g).to(tdt) if elems else torch.empty(0, dtype=tdt, device="cuda")

    op_ = _lib.i64_array(offs)
    sets = []
    for _ in range(nsets):
        stages = [filled(relems) for _ in range(NSRC - 1)]
        own, out = filled(relems), torch.empty(relems, dtype=tdt, device="cuda")
        # the own slices and the outputs lie at the region's offsets of their arenas: 256-B boundaries
        sets.append({
            "keep": (stages, own, out),
            "outs": _lib.ptr_array([out.data_ptr() + o for o in offs]),
            "owns": _lib.ptr_array([own.data_ptr() + o for o in offs]),
            "stages": _lib.ptr_array([0] + [s.data_ptr() for s in stages]),
            # the yardstick's operands: the same element count, contiguous
            "srcs": _lib.ptr_array([own.data_ptr()] + [s.data_ptr() for s in stages]),
            "dst": out.data_ptr(),
        })

    def fold_segs(i):
        s = sets[i % nsets]
        _lib.call("tips_reducescatter_fold", s["outs"][0], s["owns"][0], cp[0], op_[0], len(counts), s["stages"][0], NSRC, 0,
                  code, _lib.OP_SUM, 1.0, 1.0, sp)

    def multi_sum(i):
        s = sets[i % nsets]
        _lib.call("tips_multi_sum", s["dst"], s["srcs"][0], NSRC, n, code, sp)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        host = time.perf_counter() - t0  # what the calls themselves take: a leg is never faster than that
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3, host / steps * 1e6  # us per step: on the stream, on the host

    legs = (("fold_segs", fold_segs), ("multi_sum", multi_sum))
    for _, fn in legs:
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    us = {k: [] for k, _ in legs}
    for _ in range(reps):  # alternated: drift over the run lands on both legs alike
        for k, fn in legs:
            us[k].append(timed(fn))
    bound_us = (NSRC + 1) * n * es / PEAK * 1e6
    rec = {"shape": name, "segments": len(counts), "elements": n, "dtype": code, "nsrc": NSRC, "region_bytes": int(region),
           "payload_bytes": n * es, "launches_per_fold": -(-sum(1 for c in counts if c) // 112), "steps": steps, "warmup": warmup,
           "reps": reps, "rotating_sets": nsets, "device": torch.cuda.get_device_name(0), "bound_us_at_8TBps": round(bound_us, 2)}
    for k in us:
        v = sorted(t for t, _ in us[k])
        h = sorted(t for _, t in us[k])
        med = v[len(v) // 2]
        rec[k] = {"us_median": round(med, 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2),
                  "share_of_bound": round(bound_us / med, 4), "host_us_median": round(h[len(h) // 2], 2)}
    rec["ratio_multi_sum_over_fold_segs"] = round(rec["multi_sum"]["us_median"] / rec["fold_segs"]["us_median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    for name, counts, code in shapes():
        if args.shape and args.shape != name:
            continue
        rec = measure(name, counts, code, args.steps, args.warmup, args.reps)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
