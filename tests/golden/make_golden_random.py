"""Generate F5, the reference's (epfml/powersgd) own steps on a mixed shape set, on CPU.

Needs a checkout of the reference on the path:

    PYTHONPATH=<reference checkout> python tests/golden/make_golden_random.py

Writes ``F5_random_shapes.npz`` (data only, no pickles) into this directory: per
(rank, iterations) case the reference's initial P/Q state and, for three steps with error
feedback, its outputs and the residuals it leaves in the gradients. The inputs are rebuilt by
the test from the portable hash generator (powersgd_amd.workloads.hash_tensors), so they are not
stored. Pins ``oracle/powersgd_oracle.py`` bitwise (tests/test_oracle_golden.py).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from powersgd_amd.workloads import hash_tensors  # noqa: E402

SHAPES = [(40, 30), (40, 30), (7, 5, 2), (9,), (128, 3, 3), (5, 300)]
CASES = ((1, 2), (3, 3), (2, 1))  # (rank, num_iters_per_step)
MCR = 1.5
STEPS = 3


def fresh(case: int, step: int):
    return [torch.from_numpy(f) for f in hash_tensors(SHAPES, seed=3000 + 10 * case + step)]


def main():
    from powersgd import Config, PowerSGD

    rec = {}
    for ci, (rank, iters) in enumerate(CASES):
        ref = PowerSGD([torch.zeros(s) for s in SHAPES], Config(rank, MCR, iters, 0))
        rec[f"c{ci}_p0"] = ref._powersgd._ps_buffer.numpy().copy()
        rec[f"c{ci}_q0"] = ref._powersgd._qs_buffer.numpy().copy()
        grads = fresh(ci, 0)
        for t in range(STEPS):
            outs = ref.aggregate(grads)
            for i in range(len(SHAPES)):
                rec[f"c{ci}_s{t}_out_{i}"] = outs[i].numpy().copy()
                rec[f"c{ci}_s{t}_res_{i}"] = grads[i].numpy().copy()
            for g, f in zip(grads, fresh(ci, t + 1)):
                g.add_(f)
    np.savez_compressed(os.path.join(HERE, "F5_random_shapes.npz"), **rec)


if __name__ == "__main__":
    main()
