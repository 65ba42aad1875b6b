"""The DDP comm hook with ``PowerSGDState(residual_dtype=torch.float32)`` on a bf16 model: bit
for bit the fp32 flow on the same (bf16-rounded) gradients, and within the fp32 tolerances of
the CPU oracle.

W = 2 processes on cuda:0 over gloo, the ``_Probe`` model of tests/test_gpu_ddp_bf16.py (loss
sum_i <p_i, c_i>, so each rank's local gradient is exactly its c_i), ~10 KB buckets. Each process
holds two DDP models, stepped one after the other (the same collective order on both ranks):

* bf16 parameters, ``residual_dtype=torch.float32``, fed c_i rounded to bf16;
* fp32 parameters, a plain state, fed the same bf16-rounded c_i upcast.

Both residuals are flat fp32 buffers of one layout, both codecs the fp32 one, and the bf16
buckets are upcast exactly before ONE fp32 add: ``state.views`` must be bitwise equal, and the
bf16 model's ``p.grad`` the bf16 rounding of the fp32 model's. The residuals are also checked
against W oracle workers (oracle/multiworker.py) running free on the upcast inputs, at the fp32
tolerances TOL_STEP (first step) / TOL_FREE: the 4e-3 bf16 storage bound of
tests/test_gpu_ddp_bf16.py no longer applies to the state carried from step to step."""
import os
import tempfile

import pytest
import torch

from parity_log import check
from training_io import SHAPES, init_params, step_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_STEP, TOL_FREE = 1e-5, 1e-4
STEPS = 3
BF16 = torch.bfloat16


class _Probe(torch.nn.Module):
    def __init__(self, init):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.clone()) for p in init])

    def forward(self, cs):
        return sum((p * c).sum() for p, c in zip(self.ps, cs))


def _rel(a, b, scale) -> float:
    return float((a.detach().double().cpu() - b.double()).norm()) / max(float(scale.double().norm()), 1e-30)


def _run(rank_id, world, rank, iters):
    from torch.nn.parallel import DistributedDataParallel as DDP

    from oracle import multiworker as MW
    from oracle import powersgd_oracle as O
    from powersgd_amd import Config
    from powersgd_amd.ddp import PowerSGDState, powersgd_hook

    cfg = Config(rank, 2, iters, 0)
    models, states = [], []
    for dtype, res in ((BF16, torch.float32), (torch.float32, None)):
        model = _Probe([p.to(dtype) for p in init_params()]).to(DEV)
        ddp = DDP(model, device_ids=[0], bucket_cap_mb=0.01)
        state = PowerSGDState(cfg, params=list(model.parameters()), residual_dtype=res)
        ddp.register_comm_hook(state, powersgd_hook)
        models.append(ddp)
        states.append(state)
    lo, hi = states
    assert lo.residual.dtype == torch.float32 and all(v.dtype == torch.float32 for v in lo.views)
    assert lo.powersgd._powersgd.dtype == torch.float32  # the F32 codec over the fp32 views
    assert torch.equal(lo.powersgd._powersgd._ps_buffer, hi.powersgd._powersgd._ps_buffer)
    oracles = []
    for _ in range(world):
        st = O.policy_init([torch.zeros(s) for s in SHAPES], rank, 2, iters, 0)
        st.codec.p_flat.copy_(hi.powersgd._powersgd._ps_buffer.cpu())
        st.codec.q_flat.copy_(hi.powersgd._powersgd._qs_buffer.cpu())
        oracles.append(st)
    ora_res = [[torch.zeros(s) for s in SHAPES] for _ in range(world)]
    p_lo, p_hi = (list(m.module.parameters()) for m in models)
    for t in range(STEPS):
        fresh = [[g.to(BF16) for g in step_grads(t, w)] for w in range(world)]  # every rank's, locally
        cs = [g.to(DEV) for g in fresh[rank_id]]
        models[0](cs).backward()
        torch.cuda.synchronize()
        models[1]([c.float() for c in cs]).backward()
        torch.cuda.synchronize()
        for i in range(len(SHAPES)):
            assert p_lo[i].grad.dtype == BF16
            assert torch.equal(lo.views[i], hi.views[i]), (rank, iters, rank_id, t, i, "residual")
            assert torch.equal(p_lo[i].grad.view(torch.int16), p_hi[i].grad.to(BF16).view(torch.int16)), \
                (rank, iters, rank_id, t, i, "average")
        gc = [[r + g.float() for r, g in zip(ora_res[w], fresh[w])] for w in range(world)]
        ins = [[x.clone() for x in gc[w]] for w in range(world)]
        MW.run_workers(oracles, gc)
        for i in range(len(SHAPES)):
            scale = max((ins[w][i] for w in range(world)), key=lambda x: float(x.norm()))
            check(_rel(lo.views[i], gc[rank_id][i], scale), TOL_STEP if t == 0 else TOL_FREE, rank, iters, rank_id,
                  t, i, "ddp-fp32res-residual")
        ora_res = gc
        for p in p_lo + p_hi:
            p.grad = None


def _worker(rank_id, world, initfile, rank, iters):
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=world)
    try:
        _run(rank_id, world, rank, iters)
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("rank,iters", [(2, 2), (1, 1), (4, 3)])
def test_ddp_hook_fp32_residual_matches_fp32_flow(rank, iters):
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_worker, args=(2, os.path.join(td, "init"), rank, iters), nprocs=2, join=True)


def test_fp32_parameters_accept_float32_and_equal_the_default():
    from powersgd_amd import Config
    from powersgd_amd.ddp import PowerSGDState

    ps = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in SHAPES]
    a = PowerSGDState(Config(1, 2, 1, 0), ps, residual_dtype=torch.float32)
    b = PowerSGDState(Config(1, 2, 1, 0), ps)
    assert a.residual.dtype == b.residual.dtype == torch.float32
    assert a._code == b._code and a._bucket_code is None and b._bucket_code is None
    ps16 = [torch.nn.Parameter(torch.zeros(s, device=DEV, dtype=BF16)) for s in SHAPES]
    assert PowerSGDState(Config(1, 2, 1, 0), ps16).residual.dtype == BF16  # the default stays bf16
