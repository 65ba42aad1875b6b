"""The DDP comm hook with ``state.direct_store = True`` under ``PSGD_COMM=ipc``: the completion is
ONE library call (psgd_aggregate_ipc_dst: the codec's final pass stores the fp32 averages straight
into the parameters' views of their DDP buckets) and must equal, bit for bit, the three-stage
completion (psgd_aggregate_ipc into the output slab, then the per-bucket GATHER) on identical
models and inputs.

W = 2 processes on cuda:0, DDP over gloo, the ``_Probe`` model and the ~10 KB buckets of
tests/test_gpu_ddp_fused_ipc.py (loss sum_i <p_i, c_i>: each rank's local gradient is exactly its
own c_i, so the ranks hold different gradients). One spawn: every rank runs the three-stage model,
then the direct one (a fresh model, state and exchange session each), and leaves ``p.grad``, the
residual and P/Q of every step of both in files; the test compares the files. One warm-up step (``start_compressing_after_num_steps=1``), then two
compressing ones."""
import os

import pytest
import torch

from training_io import init_params, step_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEPS = 3
WARMUP = 1
CASES = [(2, 2), (16, 1)]  # rank x iterations: the ending after a fused k_final_odd, the matrix-core apply


class _Probe(torch.nn.Module):
    def __init__(self, init):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.clone()) for p in init])

    def forward(self, cs):
        return sum((p * c).sum() for p, c in zip(self.ps, cs))


def _bits(x):
    return x.detach().contiguous().view(torch.int32).cpu()


def _case(rank_id, rank, iters, direct):
    from torch.nn.parallel import DistributedDataParallel as DDP

    from powersgd_amd import Config
    from powersgd_amd.ddp import PowerSGDState, powersgd_hook

    model = _Probe(init_params()).to(DEV)
    ddp = DDP(model, device_ids=[0], bucket_cap_mb=0.01)
    state = PowerSGDState(Config(rank, 2, iters, WARMUP), params=list(model.parameters()))
    state.direct_store = direct
    ddp.register_comm_hook(state, powersgd_hook)
    mask = state.powersgd.is_compressed_mask
    assert any(mask) and not all(mask), mask
    codec = state.powersgd._powersgd
    params = list(model.parameters())
    rec = []
    for t in range(STEPS):
        cs = [g.to(DEV) for g in step_grads(t, rank_id)]
        applies = state.direct_store_applies()
        ddp(cs).backward()
        torch.cuda.synchronize()
        rec.append({"applies": applies, "grad": [_bits(p.grad) for p in params], "residual": _bits(state.residual),
                    "ps": _bits(codec._ps_buffer), "qs": _bits(codec._qs_buffer)})
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
        for direct in (False, True):
            recs = {f"{rank}x{iters}": _case(rank_id, rank, iters, direct) for rank, iters in CASES}
            torch.save(recs, os.path.join(outdir, f"direct{int(direct)}_rank{rank_id}.pt"))
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


def test_ddp_hook_direct_over_ipc_equals_three_stage_completion(tmp_path):
    """``p.grad`` bits, the residual and P/Q after each of 3 steps, at rank buckets 2 and 16;
    ``direct_store_applies()`` is True on compressing steps, False during warm-up and always for a
    plain state."""
    out = str(tmp_path)
    torch.multiprocessing.spawn(_worker, args=(os.path.join(out, "init"), out), nprocs=2, join=True)
    for rank_id in (0, 1):
        ref = torch.load(os.path.join(out, f"direct0_rank{rank_id}.pt"))
        one = torch.load(os.path.join(out, f"direct1_rank{rank_id}.pt"))
        for key in ref:
            assert [r["applies"] for r in ref[key]] == [False] * STEPS, (key, rank_id)
            assert [r["applies"] for r in one[key]] == [False] * WARMUP + [True] * (STEPS - WARMUP), (key, rank_id)
            assert any(bool(r["residual"].any()) for r in ref[key]), key  # the residuals are non-trivial
            for t, (x, y) in enumerate(zip(one[key], ref[key])):
                for i, (p, q) in enumerate(zip(x["grad"], y["grad"])):
                    assert torch.equal(p, q), (key, rank_id, t, i, "p.grad")
                for k in ("residual", "ps", "qs"):
                    assert torch.equal(x[k], y[k]), (key, rank_id, t, k)
    # the ranks fed different gradients: their residuals differ
    a = torch.load(os.path.join(out, "direct1_rank0.pt"))
    b = torch.load(os.path.join(out, "direct1_rank1.pt"))
    for key in a:
        assert not torch.equal(a[key][-1]["residual"], b[key][-1]["residual"]), key
