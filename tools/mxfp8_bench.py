#!/usr/bin/env python3
"""What the MXFP8 wire's three kernels cost at one rank, by tools/adasum_bench.py's
method: rotating buffer sets (no launch finds its operands in the Infinity Cache), HIP events on the
launch stream, a warm-up, medians over alternated repetitions, in one process:

  (a) quantize    tips_mxfp8_quantize of the list: reads 4 B, writes 33/32 B per element
  (b) fold8       tips_mxfp8_fold of 8 sources over one eighth of the blocks (what one rank of 8 folds):
                  (8 + 1) * 33/32 B per element of the eighth
  (c) dequantize  tips_mxfp8_dequantize into the list: reads 33/32 B, writes 4 B per element
  (d) cast16      tips_fused_allreduce_cast (float16 wire) of the same list at one rank: the cast pack
                  and the cast unpack, 6 + 6 B per element - what Compression.fp16 costs for the same job

Shapes: config 5's 214 gradient counts as one list, and one 256 MiB tensor. share = the bytes-only
bound at 8 TB/s / the median. No ratio is fixed in advance: the records say what was measured. The
collective itself (the exchange over xGMI) cannot be measured on one GPU.
Prints one JSON line per shape; --out appends them to a file (profiles/mxfp8/).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROTATE_BYTES = 1536 << 20
PEAK = 8e12


def shapes():
    from bench import resnet50_grad_sizes
    return [("config5_214_f32", [int(c) for c in resnet50_grad_sizes()]), ("1x256MiB_f32", [(256 << 20) // 4])]


def measure(name, counts, steps, warmup, reps, legs_wanted):
    import torch
    import tips_amd
    from tips_amd import _lib, ops
    tips_amd.init()
    n = sum(counts)
    elems, offs = ops.mxfp8_flat_elems(counts)
    wire_bytes, _ = ops.mxfp8_wire_bytes(elems)
    nblocks = -(-elems // 32)
    nsets = max(3, -(-ROTATE_BYTES // (4 * n + wire_bytes)))
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    cp = _lib.i64_array(counts)
    g = torch.Generator(device="cuda")

    def tensor_set(seed):
        """The list's tensors as views of one arena, each on a 256-B boundary (separate allocations' alignment)."""
        arena = torch.empty(elems, dtype=torch.float32, device="cuda")
        if seed is not None:
            g.manual_seed(seed)
            arena.normal_(generator=g)
        ts = [arena[o:o + c] for o, c in zip(offs, counts)]
        return arena, ts, _lib.ptr_array([t.data_ptr() for t in ts])

    ins = [tensor_set(k + 1) for k in range(nsets)]
    outs = [tensor_set(None) for _ in range(nsets)]
    wires = [torch.empty(wire_bytes, dtype=torch.uint8, device="cuda") for _ in range(max(nsets, 8))]
    for k, w in enumerate(wires):  # every wire buffer holds a quantised list before fold / dequantize read it
        _lib.call("tips_mxfp8_quantize", ins[k % nsets][2][0], cp[0], len(counts), w.data_ptr(), sp)
    fold_dst = torch.empty(wire_bytes, dtype=torch.uint8, device="cuda")
    fold_srcs = _lib.ptr_array([w.data_ptr() for w in wires[:8]])
    eighth = nblocks // 8

    def quantize(i):
        _lib.call("tips_mxfp8_quantize", ins[i % nsets][2][0], cp[0], len(counts), wires[i % nsets].data_ptr(), sp)

    def fold8(i):  # another eighth every step: 8 steps read the 8 whole source buffers
        _lib.call("tips_mxfp8_fold", fold_dst.data_ptr(), fold_srcs[0], 8, elems, (i % 8) * eighth, eighth, sp)

    def dequantize(i):
        _lib.call("tips_mxfp8_dequantize", outs[i % nsets][2][0], cp[0], len(counts), wires[i % nsets].data_ptr(), 1.0, sp)

    def cast16(i):
        _lib.call("tips_fused_allreduce_cast", ins[i % nsets][2][0], outs[i % nsets][2][0], cp[0], len(counts),
                  _lib.FLOAT32, _lib.FLOAT16, sp)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(steps):
            fn(i)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3  # us per step

    all_legs = (("quantize", quantize), ("fold8", fold8), ("dequantize", dequantize), ("cast16", cast16))
    legs = [(k, f) for k, f in all_legs if k in legs_wanted]
    for _, fn in legs:
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    us = {k: [] for k, _ in legs}
    for _ in range(reps):  # alternated: drift over the run lands on every leg alike
        for k, fn in legs:
            us[k].append(timed(fn))
    rec = {"shape": name, "tensors": len(counts), "elements": n, "flat_elements": elems, "wire_bytes": wire_bytes,
           "steps": steps, "warmup": warmup, "reps": reps, "rotating_sets": nsets, "device": torch.cuda.get_device_name(0)}
    bound_bytes = {"quantize": n * (4 + 33 / 32), "fold8": eighth * 32 * 9 * 33 / 32, "dequantize": n * (33 / 32 + 4),
                   "cast16": n * 12}
    for k in us:
        v = sorted(us[k])
        med = v[len(v) // 2]
        rec[k] = {"us_median": round(med, 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2),
                  "bound_us_at_8TBps": round(bound_bytes[k] / PEAK * 1e6, 2),
                  "share_of_bound": round(bound_bytes[k] / PEAK * 1e6 / med, 4)}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="quantize,fold8,dequantize,cast16")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    for name, counts in shapes():
        if args.shape and args.shape != name:
            continue
        rec = measure(name, counts, args.steps, args.warmup, args.reps, args.legs.split(","))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
