"""-m gpu: the MXFP8 error-feedback collectives across real processes, one RCCL rank each on the one
GPU (the environment, the pattern and the timeout of tests/test_gpu_mxfp8_procs.py; at most 8 processes).

p = 2, 3, 8, three steps each with the state carried forward: tips_allreduce_mxfp8_ef over 70001
elements (out of place, and in place with the factor 1 / p) and over 100 elements (4 blocks: every
rank but 0 owns an empty chunk and never touches its owner residual), the flat list call over the
20-tensor list of the Adasum process test, and allreduce_grads(compression=<MXFP8ErrorFeedback>) -
every rank's outputs bit for bit the restatement's collective_ef (tests/mxfp8_ef_util.py), one sha1
across the ranks, every rank's own state bit for bit. A feedback call on rank 0 against the plain
call on the others, and a state 4 bytes short on rank 1: TIPS_ERR_MISMATCH on every rank, the
states untouched, and the job goes on."""
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


def run_ef_job(p, cases, timeout=300):
    """One process per rank under one timeout, as test_gpu_mxfp8_procs.run_mxfp8_job: a job that runs
    out of it is reported with every rank's stack (faulthandler) and never started again."""
    assert p <= 8
    env = dict(os.environ, TIPS_VERBOSE="1")
    env.update(rccl_env("auto"))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "mxfp8_ef_worker.py"), str(r), str(p), json.dumps(cases)],
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


def ef_cases():
    return [
        {"kind": "single", "counts": [70001], "seed": 10},
        {"kind": "single", "counts": [70001], "seed": 11, "inplace": True, "factor": "1/p", "new_inputs": 1},
        {"kind": "single", "counts": [100], "seed": 12},  # 4 blocks: chunk 0 is all of them
        {"kind": "flat", "counts": LIST20, "seed": 20, "factor": 0.5},
        {"kind": "grads", "counts": LIST20[:8], "seed": 30},
        {"kind": "kind_mismatch", "counts": [300], "seed": 40},
        {"kind": "short_state", "counts": [300], "seed": 41},
        {"kind": "single", "counts": [300], "seed": 42},  # the job goes on
    ]


@pytest.mark.parametrize("p", [2, 3, 8])
def test_mxfp8_ef_across_processes(gpu, p):
    cases = ef_cases()
    for c in cases:
        if c.get("factor") == "1/p":
            c["factor"] = 1.0 / p
    results = run_ef_job(p, cases)
    assert sorted(res["rank"] for res in results) == list(range(p))
    bad = ["rank %d: %r" % (res["rank"], c) for res in results for c in res["results"] if not c["ok"]]
    assert not bad, "\n".join(bad[:12])
    for i, c in enumerate(cases):
        per_rank = [res["results"][i] for res in sorted(results, key=lambda r: r["rank"])]
        if "sha1" in per_rank[0]:  # the same output bits on every rank, and something was carried
            assert len({r["sha1"] for r in per_rank}) == 1, (c, per_rank)
            assert all(r["state_nonzero"] for r in per_rank), (c, per_rank)
        if c["kind"] == "kind_mismatch":
            assert all(r["rc"] == -7 and "Mismatched MXFP8" in r["error"] for r in per_rank), per_rank
        if c["kind"] == "short_state":
            assert all(r["rc"] == -7 for r in per_rank), per_rank
            assert "ef_bytes" in per_rank[1]["error"], per_rank
            assert all("refused its arguments" in r["error"] for k, r in enumerate(per_rank) if k != 1), per_rank
