#!/usr/bin/env python3
"""What the ordered row sum (tips_rows_sum) costs, by tools/minmax_bench.py's method:
rotating buffer sets larger than the Infinity Cache (no launch finds its operands there), HIP events
on the launch stream, a warm-up, and in one process, alternated repetition by repetition:

  (a) rows_sum    tips_rows_sum: memset + count + scan + place + order + fold, every row of the
                  table written once
  (b) index_add   torch: table.zero_() then table.index_add_(0, indices, values) - what
                  sparse_as_dense=True runs today (float atomics: its bits change from run to run)
  (c) copy        copy_buf_kernel (tips_allreduce at one rank, out of place) over 256 MiB: the copy
                  rate of this process, for the bytes-only bound

The bound: the row sum must read G * D * es bytes of values and write R * D * es bytes of table;
bound_us = those bytes at (c)'s measured rate (bytes read + bytes written per second). share =
bound_us / rows_sum's median. No ratio is fixed in advance: the records say what was measured.

Shapes: G = 64 Ki entries into R = 1 Mi rows at D = 128 f32; the same at D = 16; G = 1 Mi, R = 64 Ki,
D = 64 bf16 - each with uniform and with Zipf-like (exponent 1.2) indices. Each (shape, indices) runs
in a child process of its own under a time limit (--shape / --dist run one in this process); --legs
restricts the legs (a kernel trace of the row sum alone runs `--legs rows_sum` under the profiler).
Prints one JSON line per run; --out appends them to a file (profiles/sparse/).
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "g64k_r1m_d128_f32": (64 << 10, 1 << 20, 128, "f32"),
    "g64k_r1m_d16_f32": (64 << 10, 1 << 20, 16, "f32"),
    "g1m_r64k_d64_bf16": (1 << 20, 64 << 10, 64, "bf16"),
}
DISTS = ("uniform", "zipf")
ROTATE_BYTES = 640 << 20  # one rotation through the sets moves more than the 256 MiB Infinity Cache holds
COPY_MIB = 256


def make_indices(dist, G, R, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    if dist == "uniform":
        return rng.integers(0, R, G, dtype=np.int64)
    return ((rng.zipf(1.2, G) - 1) % R).astype(np.int64)


def measure(shape, dist, steps, warmup, reps, legs_wanted):
    import numpy as np
    import torch
    from tips_amd import _lib
    G, R, D, dt = SHAPES[shape]
    code, tdt, es = (_lib.FLOAT32, torch.float32, 4) if dt == "f32" else (_lib.BFLOAT16, torch.bfloat16, 2)
    need = _lib.lib().tips_rows_sum_workspace(R, G)
    per_set = (G + R) * D * es + 8 * G + need
    nsets = max(4, -(-ROTATE_BYTES // per_set))
    g = torch.Generator(device="cuda")
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    sets = []
    seg_max = 0
    for k in range(nsets):
        g.manual_seed(k + 1)
        vals = torch.empty(G, D, dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=g).to(tdt)
        idx_h = make_indices(dist, G, R, 100 + k)
        seg_max = max(seg_max, int(np.bincount(idx_h).max()))
        idx = torch.from_numpy(idx_h).cuda()
        table = torch.empty(R, D, dtype=tdt, device="cuda")
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
        sets.append((vals, idx, table, ws))
    cn = COPY_MIB << 18  # f32 elements
    copies = [(torch.empty(cn, device="cuda").uniform_(-1.0, 1.0, generator=g), torch.empty(cn, device="cuda"))
              for _ in range(4)]

    def rows_sum(i):
        vals, idx, table, ws = sets[i % nsets]
        _lib.call("tips_rows_sum", table.data_ptr(), R, D, vals.data_ptr(), idx.data_ptr(), G, code, 1.0, 1.0,
                  ws.data_ptr(), need, sp)

    def index_add(i):
        vals, idx, table, _ = sets[i % nsets]
        table.zero_()
        table.index_add_(0, idx, vals)

    def copy(i):
        src, dst = copies[i % 4]
        _lib.call("tips_allreduce", src.data_ptr(), dst.data_ptr(), cn, _lib.FLOAT32, _lib.OP_SUM, sp)

    def timed(fn, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(count):
            fn(i)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / count * 1e3  # us per step

    legs = [(n, f) for n, f in (("rows_sum", rows_sum), ("index_add", index_add), ("copy", copy)) if n in legs_wanted]
    for _, fn in legs:
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(reps):  # alternated: drift over the run lands on every leg alike
        for name, fn in legs:
            us[name].append(timed(fn, steps))
    rec = {"shape": shape, "G": G, "R": R, "D": D, "dtype": dt, "indices": dist, "largest_segment": seg_max,
           "steps": steps, "warmup": warmup, "reps": reps, "rotating_sets": nsets, "set_bytes": per_set,
           "device": torch.cuda.get_device_name(0)}
    for name in us:
        v = sorted(us[name])
        rec[name] = {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2),
                     "us_all": [round(x, 2) for x in us[name]]}
    if "rows_sum" in us and "index_add" in us:
        rec["index_add_over_rows_sum"] = round(rec["index_add"]["us_median"] / rec["rows_sum"]["us_median"], 3)
    if "copy" in us:
        rate = 2 * cn * 4 / (rec["copy"]["us_median"] * 1e-6)  # bytes read + written per second
        rec["copy_GBps"] = round(rate / 1e9, 1)
        rec["bound_bytes"] = (G + R) * D * es
        rec["bound_us"] = round(rec["bound_bytes"] / rate * 1e6, 2)
        if "rows_sum" in us:
            rec["share_of_byte_bound"] = round(rec["bound_us"] / rec["rows_sum"]["us_median"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help="one shape, in this process (with --dist)")
    ap.add_argument("--dist", choices=DISTS, default="uniform")
    ap.add_argument("--legs", default="rows_sum,index_add,copy")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per run (child processes)")
    args = ap.parse_args()
    if args.shape is None:
        for shape in SHAPES:  # a fresh process per run, each under its own time limit; the first failure ends it all
            for dist in DISTS:
                cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--dist", dist, "--steps", str(args.steps),
                       "--warmup", str(args.warmup), "--reps", str(args.reps), "--legs", args.legs]
                cmd += ["--out", args.out] if args.out else []
                rc = subprocess.run(cmd, timeout=args.timeout).returncode
                if rc != 0:
                    sys.exit("%s / %s exited %d" % (shape, dist, rc))
        return
    import torch
    import tips_amd
    if not torch.cuda.is_available():
        sys.exit("sparse_bench needs a HIP device: there is nothing to time without one")
    torch.cuda.set_device(0)
    tips_amd.init()
    rec = measure(args.shape, args.dist, args.steps, args.warmup, args.reps, set(args.legs.split(",")))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
