"""The DDP hook at ranks 33-128 under a real ``DistributedDataParallel``: ``direct_store = True`` (fp32,
psgd_aggregate_comm_dst_wide) against a plain state, and bf16 parameters over an fp32 residual with ``fused=True``
(psgd_aggregate_mixed_comm_dst_wide) against ``fused=False``, on raw bits. The children, models and comparisons are
those of tests/test_gpu_ddp_direct.py and tests/test_gpu_ddp_fused.py (a 1-rank gloo group, the stand-in collective
library as each state's communicator, every observable after every step), run on tests/test_gpu_wide_dst.py's shapes."""
import pytest
import torch

import test_gpu_ddp_direct
import test_gpu_ddp_fused
from test_gpu_wide_dst import SHAPES

pytestmark = pytest.mark.gpu


def _hook(_, init, bf16):
    from powersgd_amd import Config

    mod = test_gpu_ddp_fused if bf16 else test_gpu_ddp_direct
    mod.SHAPES, mod.STEPS = SHAPES, 4  # in this child only; four steps: warm-up, DDP's bucket rebuild, both parities
    on, off = ((0, 1), (0, 0)) if bf16 else (True, False)
    ch = mod._Child(init)
    try:
        for attrs in ({}, {"max_grad_norm": 1.0}, {"skip_nonfinite": True}):  # the last two keep the three stages
            def model(*a):
                ddp, state = mod._Child.model(ch, *a)
                assert state.powersgd._powersgd._plan.is_wide()
                for k, v in attrs.items():
                    setattr(state, k, v)
                return ddp, state

            ch.model = model
            for rank, world in ((64, 3), (128, 3), (64, 1), (128, 1)) if not attrs else ((64, 3),):
                want = [off] + [off if attrs else on] * 3  # one warm-up step
                ch.compare(Config(rank, 0.7, 2, 1), world, want, (bf16, rank, world, attrs))
    finally:
        ch.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_real_ddp_wide_one_call_equals_three_stages_bitwise(bf16, tmp_path):
    """Ranks 64 and 128, I = 2, world 3 and 1: ``direct_store_applies()`` / ``fused_folds()`` read True / (0, 1) on
    compressing steps, False / (0, 0) in warm-up and with ``max_grad_norm`` or ``skip_nonfinite``; the run equals its twin."""
    torch.multiprocessing.spawn(_hook, args=(f"file://{tmp_path}/store", bf16), nprocs=1, join=True)
