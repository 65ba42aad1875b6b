"""A plain bench.py run (no --full) on the GPU: the result line carries the headline and none of
the --full blocks, --steps sets the timed steps, and --dump-outputs writes the last timed step's
outputs, identical from run to run (seeded inputs and codec state), so two builds can be compared
file by file. The smallest config (one 1024 x 1024 matrix) keeps the two runs short."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "warm", "post_backward", "rank4", "cfg4", "cfg5", "w_gt1_path", "cpu_baseline",
             "ipc_exchange", "multi_gpu_parity")


def _plain(dump):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PSGD_COMM")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "cfg1_1024sq_r1", "--dump-outputs", dump], env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_line_and_reproducible_dump(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _plain(a)
    _plain(b)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps: bytes of one step / time of one step.
    # The line rounds ms_per_step to 4 decimals and value to 3, so the unrounded time lies within
    # 5e-5 ms of the printed one and value within 5e-4 GB/s of bytes / that time.
    byts = line["config"]["gradient_bytes_per_rank"]
    ms = line["ms_per_step"]
    assert ms > 5e-5
    lo, hi = byts / ((ms + 5e-5) * 1e-3) / 1e9 - 5e-4, byts / ((ms - 5e-5) * 1e-3) / 1e9 + 5e-4
    print("value", line["value"], "bounds from ms_per_step", lo, hi)
    assert lo * (1 - 1e-9) <= line["value"] <= hi * (1 + 1e-9)
    assert not set(FULL_ONLY) & set(line), sorted(set(FULL_ONLY) & set(line))
    names = sorted(os.listdir(a))
    assert names == ["out_0000.npy", "residual_0000.npy"] and names == sorted(os.listdir(b))
    for name in names:
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert x.dtype == np.float32 and x.shape == (1024 * 1024,)
        assert np.isfinite(x).all() and np.abs(x).max() > 0
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("steps", [1, 5])
def test_steps_sets_the_timed_calls(steps, monkeypatch):
    """--steps K: the timed region of a plain run makes exactly K aggregate calls (counted, not read
    back from the line), after exactly --warmup calls outside it, and nothing is timed besides."""
    import argparse

    import torch

    import bench
    import powersgd_amd

    calls, spans = [], []
    aggregate, timed = powersgd_amd.PowerSGD.aggregate, bench.timed

    def counting(self, gradients):
        calls.append(1)
        return aggregate(self, gradients)

    def spy(fn, k, *rest):
        n0 = len(calls)
        elapsed = timed(fn, k, *rest)
        spans.append((k, n0, len(calls) - n0))
        return elapsed

    monkeypatch.setattr(powersgd_amd.PowerSGD, "aggregate", counting)
    monkeypatch.setattr(bench, "timed", spy)
    a = argparse.Namespace(steps=steps, warmup=2, sets=2, iters=None, config="cfg1_1024sq_r1", full=False)
    line = bench.measure(a, a.config, 1, 0, torch.device("cuda:0"), "nccl", "both")
    assert spans == [(steps, 2, steps)]  # one timed loop: asked for K, after 2 warm-up calls, made K
    assert len(calls) == 2 + steps
    assert line["steps"] == steps and line["ms_per_step"] > 0
