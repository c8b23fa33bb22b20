#!/usr/bin/env python3
"""What the MXFP8 reduce-scatter's kernels cost at one rank, by tools/reducescatter_bench.py's
method: rotating buffer sets (no launch finds its operands in the Infinity Cache), HIP events on the
launch stream, a warm-up, medians over alternated repetitions, in one process:

  mx_fold        tips_reducescatter_mxfp8_fold at nsrc = 8, own_pos = 0: 7 wire buffers and the own f32
                 slices read, the f32 outputs written - 4 + 4 + 7 * 33/32 B per element
  plain_fold     tips_reducescatter_fold at nsrc = 8 on the same element counts: 7 f32 stages and the own
                 slices read, the outputs written - 36 B per element. Unchanged by this feature: the yardstick
  peer_quantize  tips_mxfp8_quantize over the 7 peer regions' slices as one list (what the collective
                 launches before its exchange): 4 B read and 33/32 B written per peer element

Shapes: (a) one segment of 8 Mi f32 elements; (b) slice 0 of 8 of config 5's 214 gradients (each taken
as a [count] tensor, so slice 0 holds ceil(count / 8) elements), own slices and outputs each on a 256-B
boundary. share = the leg's own bytes-only bound at 8 TB/s / its median. No target is fixed in advance:
the records say what was measured. The collective itself (the exchange over xGMI) and every N > 1 rate
cannot be measured on one GPU. Prints one JSON line per shape; --out appends them to a file
(profiles/reducescatter_mxfp8/).
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
    grads = [int(c) for c in resnet50_grad_sizes()]
    return [("1x8Mi_f32", [8 << 20]), ("config5_214_slice0of8_f32", [-(-c // NSRC) for c in grads])]


def measure(name, counts, steps, warmup, reps):
    import torch
    import tips_amd
    from tips_amd import _lib, ops
    tips_amd.init()
    n, nseg = sum(counts), len(counts)
    cp, ep = _lib.i64_array(counts), _lib.i64_array([1] * nseg)
    offs = (ctypes.c_int64 * nseg)()
    region = _lib.call("tips_reducescatter_layout", cp[0], ep[0], nseg, _lib.FLOAT32, 1, 0, offs)  # bytes: the plain fold's stages
    offs = [int(o) for o in offs]
    elems, mx_offs = ops.mxfp8_flat_elems(counts)  # flat elements: the wire buffers'
    assert [4 * o for o in mx_offs] == offs, "the two layouts place the slices alike below one fusion bucket"
    wire_bytes, _ = ops.mxfp8_wire_bytes(elems)
    relems = -(-region // 256) * 256 // 4
    peers = NSRC - 1
    send_elems, _ = ops.mxfp8_flat_elems(counts * peers)
    send_bytes, _ = ops.mxfp8_wire_bytes(send_elems)
    per_set = (NSRC + 1) * relems * 4 + peers * wire_bytes + send_bytes
    nsets = max(3, -(-ROTATE_BYTES // per_set))
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(19)

    def filled(k):
        return torch.empty(k, dtype=torch.float32, device="cuda").normal_(generator=g)

    op_ = _lib.i64_array(offs)
    qcp = _lib.i64_array(counts * peers)
    sets = []
    for _ in range(nsets):
        stages = [filled(relems) for _ in range(peers)]
        own, out = filled(relems), torch.empty(relems, dtype=torch.float32, device="cuda")
        # the peers' wires: each stage's slices quantised under the region's layout (not timed)
        wires = [ops.mxfp8_quantize([s[o // 4:o // 4 + c] for o, c in zip(offs, counts)]) for s in stages]
        send = torch.empty(send_bytes, dtype=torch.uint8, device="cuda")
        sets.append({
            "keep": (stages, own, out, wires, send),
            "outs": _lib.ptr_array([out.data_ptr() + o for o in offs]),
            "owns": _lib.ptr_array([own.data_ptr() + o for o in offs]),
            "stages": _lib.ptr_array([0] + [s.data_ptr() for s in stages]),
            "wires": _lib.ptr_array([0] + [w.data_ptr() for w in wires]),
            # the peer quantise reads the stages as this rank's slices for its 7 peers
            "qins": _lib.ptr_array([s.data_ptr() + o for s in stages for o in offs]),
            "send": send.data_ptr(),
        })
    torch.cuda.synchronize()

    def mx_fold(i):
        s = sets[i % nsets]
        _lib.call("tips_reducescatter_mxfp8_fold", s["outs"][0], s["owns"][0], cp[0], nseg, s["wires"][0], NSRC, 0, 1.0, sp)

    def plain_fold(i):
        s = sets[i % nsets]
        _lib.call("tips_reducescatter_fold", s["outs"][0], s["owns"][0], cp[0], op_[0], nseg, s["stages"][0], NSRC, 0,
                  _lib.FLOAT32, _lib.OP_SUM, 1.0, 1.0, sp)

    def peer_quantize(i):
        s = sets[i % nsets]
        _lib.call("tips_mxfp8_quantize", s["qins"][0], qcp[0], nseg * peers, s["send"], sp)

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

    legs = (("mx_fold", mx_fold), ("plain_fold", plain_fold), ("peer_quantize", peer_quantize))
    for _, fn in legs:
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    us = {k: [] for k, _ in legs}
    for _ in range(reps):  # alternated: drift over the run lands on every leg alike
        for k, fn in legs:
            us[k].append(timed(fn))
    live = sum(1 for c in counts if c)
    bytes_of = {"mx_fold": n * (4 + 4 + peers * 33 / 32), "plain_fold": n * 4 * (NSRC + 1), "peer_quantize": peers * n * (4 + 33 / 32)}
    launches = {"mx_fold": -(-live // 80), "plain_fold": -(-live // 112), "peer_quantize": -(-(live * peers) // 48)}
    rec = {"shape": name, "segments": nseg, "elements": n, "nsrc": NSRC, "flat_elems": elems, "wire_bytes": wire_bytes,
           "send_wire_bytes": send_bytes, "steps": steps, "warmup": warmup, "reps": reps, "rotating_sets": nsets,
           "device": torch.cuda.get_device_name(0)}
    for k in us:
        v = sorted(t for t, _ in us[k])
        h = sorted(t for _, t in us[k])
        med, bound_us = v[len(v) // 2], bytes_of[k] / PEAK * 1e6
        rec[k] = {"us_median": round(med, 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2), "bytes": int(bytes_of[k]),
                  "bound_us_at_8TBps": round(bound_us, 2), "share_of_bound": round(bound_us / med, 4),
                  "host_us_median": round(h[len(h) // 2], 2), "launches": launches[k]}
    rec["ratio_plain_fold_over_mx_fold"] = round(rec["plain_fold"]["us_median"] / rec["mx_fold"]["us_median"], 4)
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
    for name, counts in shapes():
        if args.shape and args.shape != name:
            continue
        rec = measure(name, counts, args.steps, args.warmup, args.reps)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
