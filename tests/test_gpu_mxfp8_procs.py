"""-m gpu: the MXFP8 collectives across real processes, one RCCL rank each on the one GPU (the
environment of tests/test_gpu_rccl_procs.py; at most 8 processes).

p = 2, 3, 4, 8: tips_allreduce_mxfp8 over 1, 4099 and 70001 elements (out of place and in place, one
with the factor 1 / p) and the flat list call over the 20-tensor list of the Adasum process test -
every rank bit for bit the restatement's collective (tests/mxfp8_util.py), one sha1 across the ranks.
A rank with another count list: TIPS_ERR_MISMATCH on every rank, and the job goes on. A rank whose
input is host memory: its own TIPS_ERR_UNSUPPORTED there, TIPS_ERR_MISMATCH ("refused its
arguments") on every other rank, nobody waits in the exchange, and the job goes on. p = 2 also
through allreduce(compression=Compression.fp8) and allreduce_grads(compression=Compression.fp8) -
fused, unfused, op=Average under set_op_scaling(True), and a mixed list whose members that are not
float32 device tensors equal the Compression.none result."""
import json
import os
import signal
import subprocess
import sys
import time

import pytest

from test_gpu_adasum_procs import LIST20
from test_gpu_rccl_procs import rccl_env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def run_mxfp8_job(p, cases, timeout=300):
    """One process per rank under one timeout; a job that runs out of it is reported with every rank's
    stack (faulthandler) and never started again."""
    assert p <= 8
    env = dict(os.environ, TIPS_VERBOSE="1")
    env.update(rccl_env("auto"))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "mxfp8_worker.py"), str(r), str(p), json.dumps(cases)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(p)]
    outs = []
    try:
        for pr in procs:
            o, e = pr.communicate(timeout=timeout)
            outs.append((pr.returncode, o, e))
    except subprocess.TimeoutExpired:
        for pr in procs:
            if pr.poll() is None:
                pr.send_signal(signal.SIGUSR1)
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


def mxfp8_cases(p):
    cases = [
        {"kind": "single", "counts": [70001], "seed": 10},
        {"kind": "single", "counts": [4099], "seed": 11, "inplace": True},
        {"kind": "single", "counts": [1], "seed": 12},  # chunks of zero blocks on all ranks but one
        {"kind": "single", "counts": [1], "seed": 13, "inplace": True},
        {"kind": "single", "counts": [70001], "seed": 14, "inplace": True, "factor": 1.0 / p},
        {"kind": "single", "counts": [4099], "seed": 15, "factor": 1.0 / p},
        {"kind": "flat", "counts": LIST20, "seed": 20},
        {"kind": "flat", "counts": LIST20, "seed": 21, "factor": 1.0 / p},
    ]
    if p == 2:
        cases.append({"kind": "python", "counts": [4099], "seed": 41})
        cases.append({"kind": "grads", "counts": LIST20[:8], "seed": 43})
        cases.append({"kind": "grads_unfused", "counts": [5, 300, 4099], "seed": 44})
        cases.append({"kind": "grads_avg", "counts": [65, 1000, 4099, 3], "seed": 45})
        cases.append({"kind": "mixed", "counts": [300, 129, 77, 4099], "seed": 46})
    cases.append({"kind": "mismatch", "counts": [40, 50, 60], "seed": 50})
    cases.append({"kind": "refused", "counts": [300], "seed": 52})
    cases.append({"kind": "single", "counts": [300], "seed": 51})  # the job goes on
    return cases


def check(results, p, cases):
    assert sorted(res["rank"] for res in results) == list(range(p))
    bad = ["rank %d: %r" % (res["rank"], c) for res in results for c in res["results"] if not c["ok"]]
    assert not bad, "\n".join(bad[:12])
    for i, c in enumerate(cases):
        per_rank = [res["results"][i] for res in results]
        if "sha1" in per_rank[0]:
            assert len({r["sha1"] for r in per_rank}) == 1, (c, per_rank)
        if c["kind"] == "mismatch":
            assert all(r["rc"] == -7 for r in per_rank), per_rank
        if c["kind"] == "refused":  # rank 1 refused its own input; the others hear of it
            assert [r["rc"] for r in per_rank] == [-5 if k == 1 else -7 for k in range(p)], per_rank
            assert "host memory" in per_rank[1]["error"], per_rank
            assert all("refused its arguments" in r["error"] for k, r in enumerate(per_rank) if k != 1), per_rank


@pytest.mark.parametrize("p", [2, 3, 4, 8])
def test_mxfp8_across_processes(gpu, p):
    cases = mxfp8_cases(p)
    check(run_mxfp8_job(p, cases), p, cases)
