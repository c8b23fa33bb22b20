"""-m gpu: tips_sparse_allreduce across real processes, one RCCL rank each on the one GPU (the
environment of tests/test_gpu_rccl_procs.py; at most 3 processes).

Every rank brings a different number of entries, one rank none at all; index sets that overlap
(every rank names the same popular rows) and that are disjoint (rank r names rows r modulo p); f32,
bf16 and i64; op=Average with a predivision factor. Every rank must return the bits of
tests/sparse_util.py on the concatenation of the ranks' entries in rank order, and therefore the
bits of every other rank. A rank whose rows have another length makes every rank's call fail with
TIPS_ERR_MISMATCH before any entries are exchanged, and the job carries on. A rank whose dense_out
is host memory gets its own TIPS_ERR_UNSUPPORTED, every other rank TIPS_ERR_MISMATCH ("refused its
arguments"), nobody waits in the exchange, and a SUM allreduce afterwards still works."""
import json
import os
import signal
import subprocess
import sys
import time

import pytest

from gpu_util import BF16, F32, I64
from test_gpu_rccl_procs import rccl_env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def run_sparse_job(p, cases, timeout=300):
    assert p <= 3
    env = dict(os.environ, TIPS_VERBOSE="1")
    env.update(rccl_env("auto"))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "sparse_worker.py"), str(r), str(p), json.dumps(cases)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(p)]
    outs = []
    try:
        for pr in procs:
            o, e = pr.communicate(timeout=timeout)
            outs.append((pr.returncode, o, e))
    except subprocess.TimeoutExpired:
        for pr in procs:
            if pr.poll() is None:
                pr.send_signal(signal.SIGUSR1)  # (faulthandler: where every thread stands)
        time.sleep(2)
        tails = []
        for r, pr in enumerate(procs):
            pr.kill()
            o, e = pr.communicate()
            tails.append("rank %d (rc %s):\n%s\n--- stdout:\n%s" % (r, pr.returncode, e[-4000:], o[-2000:]))
        raise AssertionError("job timed out after %d s\n%s" % (timeout, "\n".join(tails)))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    results = []
    for r, (rc, o, e) in enumerate(outs):
        assert rc == 0, "rank %d exited %d:\n%s\n--- stdout:\n%s" % (r, rc, e[-3000:], o[-3000:])
        results.append(json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]))
    return results


def sparse_cases(p):
    ns = {2: [[700, 0], [0, 333], [257, 64]], 3: [[700, 0, 65], [1, 5000, 0], [64, 257, 300]]}[p]
    cases = []
    for k, (dtype, D) in enumerate(((F32, 16), (BF16, 24), (I64, 5), (F32, 7))):
        for sets in ("overlap", "disjoint"):
            cases.append({"dtype": dtype, "D": D, "rows": 200, "ns": ns[(k + (sets == "disjoint")) % len(ns)], "sets": sets,
                          "seed": 10 * k + len(sets), "coalesced": sets == "overlap" and dtype == F32})
    cases.append({"dtype": F32, "D": 12, "rows": 64, "ns": ns[0], "sets": "overlap", "seed": 91, "average": True,
                  "predivide": 3.0})
    cases.append({"dtype": BF16, "D": 8, "rows": 64, "ns": ns[1], "sets": "overlap", "seed": 92, "average": True,
                  "predivide": 1.0})
    cases.append({"dtype": F32, "D": 4, "rows": 16, "ns": [0] * p, "sets": "overlap", "seed": 93})  # nobody has entries
    cases.append({"dtype": F32, "D": 6, "rows": 32, "ns": ns[2], "sets": "overlap", "seed": 94, "mismatch": True})
    cases.append({"dtype": F32, "D": 16, "rows": 8, "ns": [4] * p, "sets": "overlap", "seed": 96, "refused": True})
    cases.append({"dtype": F32, "D": 6, "rows": 32, "ns": ns[2], "sets": "overlap", "seed": 95})  # the job goes on
    return cases


@pytest.mark.parametrize("p", [2, 3])
def test_sparse_allreduce_across_processes(gpu, p):
    cases = sparse_cases(p)
    results = run_sparse_job(p, cases)
    assert sorted(res["rank"] for res in results) == list(range(p))
    bad = ["rank %d: %r" % (res["rank"], c) for res in results for c in res["results"] if not c["ok"]]
    assert not bad, "\n".join(bad[:12])
    for i, c in enumerate(cases):
        per_rank = [res["results"][i] for res in results]
        if c.get("mismatch"):
            assert all(r["rc"] == -7 for r in per_rank), per_rank
        elif c.get("refused"):  # rank 1 refused its own dense_out; the others hear of it
            assert [r["rc"] for r in per_rank] == [-5 if k == 1 else -7 for k in range(p)], per_rank
            assert "host memory" in per_rank[1]["error"], per_rank
            assert all("refused its arguments" in r["error"] for k, r in enumerate(per_rank) if k != 1), per_rank
        else:
            assert len({r["sha1"] for r in per_rank}) == 1, (c, per_rank)
            assert per_rank[0]["entries"] == sum(c["ns"])
