"""The DDP comm hook with ``PowerSGDState(residual_dtype=torch.float32, fused=True)`` under
``PSGD_COMM=ipc``: the completion is ONE library call (psgd_aggregate_mixed_ipc_dst: the codec's
final pass and the last exchange store the bf16 averages straight into the parameters' views of
their DDP buckets) and must equal, bit for bit, the three-stage completion (``fused=False``:
psgd_aggregate_ipc into an fp32 slab, then the per-bucket GATHER) on identical models and inputs.

W = 2 processes on cuda:0, DDP over gloo, the ``_Probe`` model and the ~10 KB buckets of
tests/test_gpu_ddp_fp32_residual.py (loss sum_i <p_i, c_i>: each rank's local gradient is exactly
its own c_i, so the ranks hold different gradients). The fused and the three-stage run each live
in a spawn of their own and leave ``p.grad``, the residual and P/Q of every step in a file; the
test compares the files. One warm-up step (``start_compressing_after_num_steps=1``), then two
compressing ones."""
import os

import pytest
import torch

from training_io import SHAPES, init_params, step_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
STEPS = 3
WARMUP = 1
CASES = [(1, 1), (1, 2), (4, 1), (4, 2)]  # rank x iterations


class _Probe(torch.nn.Module):
    def __init__(self, init):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.clone()) for p in init])

    def forward(self, cs):
        return sum((p * c).sum() for p, c in zip(self.ps, cs))


def _bits(x):
    return x.detach().contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32).cpu()


def _case(rank_id, rank, iters, fused):
    from torch.nn.parallel import DistributedDataParallel as DDP

    from powersgd_amd import Config
    from powersgd_amd.ddp import PowerSGDState, powersgd_hook

    model = _Probe([p.to(BF16) for p in init_params()]).to(DEV)
    ddp = DDP(model, device_ids=[0], bucket_cap_mb=0.01)
    state = PowerSGDState(Config(rank, 2, iters, WARMUP), params=list(model.parameters()),
                          residual_dtype=torch.float32, fused=fused)
    ddp.register_comm_hook(state, powersgd_hook)
    mask = state.powersgd.is_compressed_mask
    assert any(mask) and not all(mask), mask
    codec = state.powersgd._powersgd
    params = list(model.parameters())
    rec = []
    for t in range(STEPS):
        cs = [g.to(BF16).to(DEV) for g in step_grads(t, rank_id)]
        folds = state.fused_folds()
        ddp(cs).backward()
        torch.cuda.synchronize()
        rec.append({"folds": folds, "grad": [_bits(p.grad) for p in params], "residual": _bits(state.residual),
                    "ps": _bits(codec._ps_buffer), "qs": _bits(codec._qs_buffer)})
        for p in params:
            p.grad = None
    assert codec._ipc_open and not codec.ipc_status()
    state.powersgd.close()
    return rec


def _worker(rank_id, initfile, outdir, fused):
    os.environ["PSGD_COMM"] = "ipc"
    torch.cuda.set_device(DEV)
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=2)
    try:
        recs = {f"{rank}x{iters}": _case(rank_id, rank, iters, fused) for rank, iters in CASES}
        torch.save(recs, os.path.join(outdir, f"fused{int(fused)}_rank{rank_id}.pt"))
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


def test_ddp_hook_fused_over_ipc_equals_three_stage_completion(tmp_path):
    """Test 7: ``p.grad`` bits, the residual and P/Q after each of 3 steps, at rank buckets 1 and 4
    and 1 / 2 iterations; ``fused_folds()`` is (0, 1) on compressing steps, (0, 0) during warm-up
    and always for ``fused=False``."""
    out = str(tmp_path)
    for fused in (False, True):
        torch.multiprocessing.spawn(_worker, args=(os.path.join(out, f"init{int(fused)}"), out, fused), nprocs=2,
                                    join=True)
    for rank_id in (0, 1):
        ref = torch.load(os.path.join(out, f"fused0_rank{rank_id}.pt"))
        one = torch.load(os.path.join(out, f"fused1_rank{rank_id}.pt"))
        for key in ref:
            assert [r["folds"] for r in ref[key]] == [(0, 0)] * STEPS, (key, rank_id)
            assert [r["folds"] for r in one[key]] == [(0, 0)] * WARMUP + [(0, 1)] * (STEPS - WARMUP), (key, rank_id)
            assert any(bool(r["residual"].any()) for r in ref[key]), key  # the residuals are non-trivial
            for t, (x, y) in enumerate(zip(one[key], ref[key])):
                for i, (p, q) in enumerate(zip(x["grad"], y["grad"])):
                    assert torch.equal(p, q), (key, rank_id, t, i, "p.grad")
                for k in ("residual", "ps", "qs"):
                    assert torch.equal(x[k], y[k]), (key, rank_id, t, k)
    # the ranks fed different gradients: their residuals differ
    a = torch.load(os.path.join(out, "fused1_rank0.pt"))
    b = torch.load(os.path.join(out, "fused1_rank1.pt"))
    for key in a:
        assert not torch.equal(a[key][-1]["residual"], b[key][-1]["residual"]), key
