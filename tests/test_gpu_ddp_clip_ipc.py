"""The DDP comm hook with ``max_grad_norm`` under ``PSGD_COMM=ipc``: ``direct_store`` (ONE library
call, psgd_aggregate_ipc_dst, followed by psgd_clip_dst at the process group's world size) must
equal, bit for bit, the three-stage completion with the same threshold (psgd_aggregate_ipc into the
slabs, psgd_clip_outputs, the per-bucket GATHER) on identical models and inputs, and both ranks must
report the same norm and coefficient bits (every rank holds the same all-reduced factors and sums).

W = 2 processes on cuda:0, DDP over gloo, set up as tests/test_gpu_ddp_direct_ipc.py does (the
``_Probe`` model, ~10 KB buckets, each rank its own gradients), rank 4 with two iterations. The
gradients of step t are scaled by 2^t. Every rank first runs a three-stage model at ``max_grad_norm =
inf`` (the norms alone); the threshold is the norm of step 2, so the compressing step 1 lies below it
and step 3 clips. One warm-up step (``start_compressing_after_num_steps=1``): it runs the three
stages, and their stream-form clip, in both models (its uncompressed averages may or may not exceed
the threshold: a rank-4 approximation holds only part of a gradient's norm)."""
import math
import os

import pytest
import torch

from test_gpu_ddp_direct_ipc import DEV, _Probe, _bits
from training_io import init_params, step_grads

pytestmark = pytest.mark.gpu
STEPS = 4
WARMUP = 1
RANK, ITERS = 4, 2


def _case(rank_id, direct, max_grad_norm):
    from torch.nn.parallel import DistributedDataParallel as DDP

    from powersgd_amd import Config
    from powersgd_amd.ddp import PowerSGDState, powersgd_hook

    model = _Probe(init_params()).to(DEV)
    ddp = DDP(model, device_ids=[0], bucket_cap_mb=0.01)
    state = PowerSGDState(Config(RANK, 2, ITERS, WARMUP), params=list(model.parameters()), max_grad_norm=max_grad_norm)
    state.direct_store = direct
    ddp.register_comm_hook(state, powersgd_hook)
    mask = state.powersgd.is_compressed_mask
    assert any(mask) and not all(mask), mask
    codec = state.powersgd._powersgd
    params = list(model.parameters())
    rec = []
    for t in range(STEPS):
        cs = [g.to(DEV) * float(2 ** t) for g in step_grads(t, rank_id)]
        applies = state.direct_store_applies()
        ddp(cs).backward()
        torch.cuda.synchronize()
        rec.append({"applies": applies, "grad": [_bits(p.grad) for p in params], "residual": _bits(state.residual),
                    "ps": _bits(codec._ps_buffer), "qs": _bits(codec._qs_buffer),
                    "norm": state.last_grad_norm.view(torch.int64).cpu().clone(),
                    "coef": state.last_clip_coef.view(torch.int64).cpu().clone()})
        for p in params:
            p.grad = None
    assert codec._ipc_open and not codec.ipc_status()
    state.powersgd.close()
    return rec


def _worker(rank_id, initfile, outdir):
    os.environ["PSGD_COMM"] = "ipc"
    torch.cuda.set_device(DEV)
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=2)
    try:
        probe = _case(rank_id, False, math.inf)
        thr = float(probe[2]["norm"].view(torch.float64))
        recs = {"probe": probe, "three": _case(rank_id, False, thr), "direct": _case(rank_id, True, thr)}
        torch.save(recs, os.path.join(outdir, f"rank{rank_id}.pt"))
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


def _f64(x):
    return float(x.view(torch.float64))


def test_ddp_hook_direct_clip_over_ipc_equals_three_stage_clip(tmp_path):
    """``p.grad`` bits, the residual, P/Q, norm and coefficient after each of 4 steps, on both ranks."""
    out = str(tmp_path)
    torch.multiprocessing.spawn(_worker, args=(os.path.join(out, "init"), out), nprocs=2, join=True)
    recs = [torch.load(os.path.join(out, f"rank{r}.pt")) for r in (0, 1)]
    for rank_id, rec in enumerate(recs):
        three, one, probe = rec["three"], rec["direct"], rec["probe"]
        assert [r["applies"] for r in three] == [False] * STEPS, rank_id
        assert [r["applies"] for r in one] == [False] * WARMUP + [True] * (STEPS - WARMUP), rank_id
        assert any(bool(r["residual"].any()) for r in three)
        for t, (x, y) in enumerate(zip(one, three)):
            for i, (p, q) in enumerate(zip(x["grad"], y["grad"])):
                assert torch.equal(p, q), (rank_id, t, i, "p.grad")
            for k in ("residual", "ps", "qs", "norm", "coef"):
                assert torch.equal(x[k], y[k]), (rank_id, t, k)
            assert torch.equal(x["norm"], probe[t]["norm"]), (rank_id, t)  # clipping never feeds back
        coefs = [_f64(r["coef"]) for r in one]
        assert coefs[1] == 1.0 and coefs[3] < 1.0, coefs
        assert all(_f64(r["coef"]) == 1.0 for r in probe)
        # step 1 is unclipped, a clipping step differs from the unclipped probe
        assert all(torch.equal(p, q) for p, q in zip(one[1]["grad"], probe[1]["grad"]))
        assert any(not torch.equal(p, q) for p, q in zip(one[3]["grad"], probe[3]["grad"]))
    # both ranks report bit-identical norm and coefficient; their residuals differ (different gradients)
    for key in ("three", "direct"):
        for t in range(STEPS):
            for k in ("norm", "coef"):
                assert torch.equal(recs[0][key][t][k], recs[1][key][t][k]), (key, t, k)
        assert not torch.equal(recs[0][key][-1]["residual"], recs[1][key][-1]["residual"]), key
