"""-m gpu: the Adasum collectives across real processes, one RCCL rank each on the one GPU (the
environment of tests/test_gpu_rccl_procs.py; at most 8 processes).

p = 2, 4, 8: tips_allreduce_adasum (out of place and in place) and the flat list call over a small
config-like list of 20 tensors with a 1-element and an empty one, f32 and bf16 - every rank bit for
bit the restatement's tree (tests/adasum_util.py), one sha1 across the ranks. p = 2 also through
allreduce(op=Adasum) and allreduce_grads(op=Adasum), fused and not. p = 3: TIPS_ERR_UNSUPPORTED on
every rank, and a SUM allreduce afterwards still works. A rank with another count list:
TIPS_ERR_MISMATCH on every rank, and the job goes on. A rank whose input is host memory: its own
TIPS_ERR_UNSUPPORTED there, TIPS_ERR_MISMATCH ("refused its arguments") on every other rank, nobody
waits in the exchange, and the job goes on."""
import json
import os
import signal
import subprocess
import sys
import time

import pytest

from gpu_util import BF16, F32
from test_gpu_rccl_procs import rccl_env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# conv / bias / norm-like sizes: odd ones, one below a wave, one element, none, several chunks
LIST20 = [1, 64, 0, 1728, 64, 36864, 128, 3, 73728, 256, 4099, 17, 147456, 512, 5, 1000, 70001, 63, 65, 8192]


def run_adasum_job(p, cases, timeout=300):
    assert p <= 8
    env = dict(os.environ, TIPS_VERBOSE="1")
    env.update(rccl_env("auto"))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "adasum_worker.py"), str(r), str(p), json.dumps(cases)],
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


def adasum_cases(p):
    cases = []
    for k, dtype in enumerate((F32, BF16)):
        cases.append({"kind": "single", "dtype": dtype, "counts": [70001], "seed": 10 + k})
        cases.append({"kind": "single", "dtype": dtype, "counts": [4099], "seed": 20 + k, "inplace": True})
        cases.append({"kind": "flat", "dtype": dtype, "counts": LIST20, "seed": 30 + k})
    if p == 2:
        cases.append({"kind": "python", "dtype": F32, "counts": [4099], "seed": 41})
        cases.append({"kind": "python", "dtype": BF16, "counts": [65], "seed": 42})
        cases.append({"kind": "grads", "dtype": F32, "counts": LIST20[:8], "seed": 43})
        cases.append({"kind": "grads_unfused", "dtype": BF16, "counts": [5, 300, 4099], "seed": 44})
    cases.append({"kind": "mismatch", "dtype": F32, "counts": [40, 50, 60], "seed": 50})
    cases.append({"kind": "refused", "dtype": F32, "counts": [300], "seed": 52})
    cases.append({"kind": "single", "dtype": F32, "counts": [1], "seed": 51})  # the job goes on
    return cases


def check(results, p, cases):
    assert sorted(res["rank"] for res in results) == list(range(p))
    bad = ["rank %d: %r" % (res["rank"], c) for res in results for c in res["results"] if not c["ok"]]
    assert not bad, "\n".join(bad[:12])
    for i, c in enumerate(cases):
        per_rank = [res["results"][i] for res in results]
        if "sha1" in per_rank[0]:
            assert len({r["sha1"] for r in per_rank}) == 1, (c, per_rank)
        if c["kind"] == "refused":  # rank 1 refused its own `in`; the others hear of it
            assert [r["rc"] for r in per_rank] == [-5 if k == 1 else -7 for k in range(p)], per_rank
            assert "host memory" in per_rank[1]["error"], per_rank
            assert all("refused its arguments" in r["error"] for k, r in enumerate(per_rank) if k != 1), per_rank


@pytest.mark.parametrize("p", [2, 4, 8])
def test_adasum_across_processes(gpu, p):
    cases = adasum_cases(p)
    check(run_adasum_job(p, cases), p, cases)


def test_three_ranks_are_refused_and_the_job_goes_on(gpu):
    cases = [{"kind": "single", "dtype": F32, "counts": [300], "seed": 1}]
    results = run_adasum_job(3, cases)
    check(results, 3, cases)
    assert all(res["results"][0]["rc"] == -5 for res in results)
