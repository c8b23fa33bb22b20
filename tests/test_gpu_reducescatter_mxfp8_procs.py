"""-m gpu: the MXFP8 reduce-scatter across real processes, one RCCL rank each on the one GPU (the
environment of tests/test_gpu_rccl_procs.py; at most 8 processes).

p = 2, 3, 8: single tensors of 1 x 1 (no rows on all ranks but one), (p - 1) x 7 (the last rank empty),
p x 33 (slices that are not 16-B aligned), 4099 x 1 and 257 x 33, each with the plain sum, Average
(through Python) and the factor 0.375 / 3; the 20-tensor list of the Adasum process test as rows, with
three 2-D members, through grouped_reducescatter; one list that mixes f32 and bf16 tensors, whose bf16
group must equal the uncompressed reduce-scatter. Every rank checks its own shards bit for bit
against the numpy restatement over all ranks' seeded inputs (tests/reducescatter_mxfp8_util.py) and its
digest against the restatement's. A rank that calls tips_grouped_reducescatter while the others call
the MXFP8 form: TIPS_ERR_MISMATCH on every rank; a rank whose input is host memory: its own
TIPS_ERR_UNSUPPORTED there, TIPS_ERR_MISMATCH "refused its arguments" elsewhere, nobody waits; after
both, a plain MXFP8 reduce-scatter still works."""
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


def run_job(p, cases, timeout=300):
    """One process per rank under one timeout; a job that runs out of it is reported with every rank's
    stack (faulthandler) and never started again."""
    assert p <= 8
    env = dict(os.environ, TIPS_VERBOSE="1")
    env.update(rccl_env("auto"))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "reducescatter_mxfp8_worker.py"), str(r), str(p), json.dumps(cases)],
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


def cases_for(p):
    shapes = [[1, 1], [p - 1, 7], [p, 33], [4099], [257, 33]]
    cases, seed = [], 0
    for s in shapes:
        for op in ("sum", "average", "factor"):
            seed += 1
            cases.append({"kind": "single", "shapes": [s], "op": op, "seed": seed, "factor": 0.375 / 3})
    grouped = [[n] for n in LIST20] + [[p + 1, 33], [3, 5, 7], [2 * p, 128]]
    for op in ("sum", "average", "factor"):
        seed += 1
        cases.append({"kind": "grouped", "shapes": grouped, "op": op, "seed": seed, "factor": 0.375 / 3})
    cases.append({"kind": "mixed", "shapes": [[p, 33], [4099], [3, 5, 7]], "seed": seed + 1})
    cases.append({"kind": "mismatch", "shapes": [[40, 1], [50, 1], [60, 1]], "seed": 90})
    cases.append({"kind": "refused", "shapes": [[300, 1]], "seed": 91})
    cases.append({"kind": "after", "shapes": [], "seed": 92})  # the job goes on
    return cases


def check(results, p, cases):
    assert sorted(res["rank"] for res in results) == list(range(p))
    bad = ["rank %d: %r" % (res["rank"], c) for res in results for c in res["results"] if not c["ok"]]
    assert not bad, "\n".join(bad[:12])
    for i, c in enumerate(cases):
        per_rank = [res["results"][i] for res in sorted(results, key=lambda r: r["rank"])]
        if "sha1_ref" in per_rank[0]:
            assert all(r["sha1"] == r["sha1_ref"] for r in per_rank), (c, per_rank)
        if c["kind"] == "mismatch":
            assert all(r["rc"] == -7 and r["error"].startswith("Mismatched") for r in per_rank), per_rank
            assert all(r["error"].startswith("Mismatched MXFP8 reduce-scatter") for k, r in enumerate(per_rank) if k != 1), per_rank
        if c["kind"] == "refused":  # rank 1 refused its own input; the others hear of it
            assert [r["rc"] for r in per_rank] == [-5 if k == 1 else -7 for k in range(p)], per_rank
            assert "host memory" in per_rank[1]["error"], per_rank
            assert all("refused its arguments" in r["error"] for k, r in enumerate(per_rank) if k != 1), per_rank


@pytest.mark.parametrize("p", [2, 3, 8])
def test_reducescatter_mxfp8_across_processes(gpu, p):
    cases = cases_for(p)
    check(run_job(p, cases), p, cases)
