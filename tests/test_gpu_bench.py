"""-m gpu: bench.py's command line at a small bucket - the plain run (the headline alone), the
outputs it dumps, and --full's check of the same steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

MIB = 1                  # the bucket (config 2's is 256 MiB): 262144 fp32 per buffer, 512 tiles of 2 KiB
N = MIB * (1 << 20) // 4


def _bench(*extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--bucket-mib", str(MIB)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _triple(torch, k):
    """bench.sum_record's k-th seeded (a, b): torch's device generator, U[-1, 1)."""
    g = torch.Generator(device="cuda")
    a, b = (torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(2))
    g.manual_seed(1 if k == 0 else 10 + 2 * k)
    a.uniform_(-1.0, 1.0, generator=g)
    g.manual_seed(2 if k == 0 else 11 + 2 * k)
    b.uniform_(-1.0, 1.0, generator=g)
    return a, b


@pytest.mark.parametrize("steps", [5, 6])
def test_plain_run_dumps_the_last_timed_steps_sum(gpu, tmp_path, steps):
    """A plain run: one line with the headline's fields, --steps timed steps, no check and no
    optional record; c.npy is the whole float32 output of the last timed step, which summed triple
    (steps - 1) % 4 of the seeded inputs: bit-exact against torch's a + b on the same seeds."""
    import torch
    d = str(tmp_path / "dump")
    line = _bench("--steps", str(steps), "--warmup", "2", "--dump-outputs", d)
    assert line["steps"] == steps and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 3 * N * 4 / (line["ms_per_step"] / 1e3) / 2**30) <= 0.01 * line["value"] + 0.01
    assert line["check"].startswith("not run") and line["cpu_baseline"] is None
    assert line["same_buffers_repeated"] is None and "configs" not in line
    assert os.listdir(d) == ["c.npy"] and line["dumped_outputs"]["c"]["elements"] == N
    c = np.load(os.path.join(d, "c.npy"))
    assert c.dtype == np.float32 and c.shape == (N,)
    a, b = _triple(torch, (steps - 1) % 4)
    assert np.array_equal(c.view(np.uint32), (a + b).cpu().numpy().view(np.uint32))


def test_full_run_checks_the_sum(gpu):
    """--full (here without the sub-records, baselines and extra legs) still checks every triple
    bit-exact and exits by that check."""
    line = _bench("--steps", "5", "--warmup", "2", "--full", "--no-sub", "--no-cpu-baseline", "--no-extras")
    assert line["check"] == "bit-exact vs torch a+b" and line["steps"] == 5
