"""``Fp32ResidualPowerSGD`` (bf16 gradients, fp32 error-feedback residual) against the existing
fp32 ``PowerSGD``, bit for bit, and against the CPU oracle.

The bitwise reference is the fp32 ``PowerSGD`` whose gradient tensors are views of one flat fp32
buffer laid out like ``Fp32ResidualPowerSGD.residual`` (same pointer alignment, so the same
kernel paths), fed ``previous residual + fresh.float()``: exactly what the new class's ADD pass
builds from the bf16 gradients. Its residuals must equal ``views``, its outputs rounded to bf16
the returned outputs, and the passed gradients must come back zeroed.

Independently, oracle/powersgd_oracle.py (W workers: oracle/multiworker.py) runs free on the
same upcast inputs: the residual within TOL_STEP of the input norm up to the first compressed
step and TOL_FREE after, the bf16 outputs within TOL_BF16 (one bf16 rounding of each element).

Inputs: tests/training_io.SHAPES and step_grads rounded to bf16; with min_compression_rate = 2
the 1-D tensors go uncompressed. World size 2 runs as two gloo processes on cuda:0, both
aggregators in each process issuing their collectives in the same order."""
import os
import tempfile

import pytest
import torch

from parity_log import check
from training_io import SHAPES, step_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_STEP, TOL_FREE, TOL_BF16 = 1e-5, 1e-4, 4e-3
BF16 = torch.bfloat16


def _rel(a, b, scale) -> float:
    return float((a.detach().double().cpu() - b.double()).norm()) / max(float(scale.double().norm()), 1e-30)


def _bits(x):
    return x.view(torch.int16)


def _run(rank_id, world, rank, iters, mcr, start, steps):
    from oracle import multiworker as MW
    from oracle import powersgd_oracle as O
    from powersgd_amd import Config, Fp32ResidualPowerSGD, PowerSGD
    from powersgd_amd.powersgd import _views

    cfg = Config(rank, mcr, iters, start)
    shapes = [torch.Size(s) for s in SHAPES]
    new = Fp32ResidualPowerSGD([torch.zeros(s, dtype=BF16, device=DEV) for s in shapes], cfg)
    assert new.residual.dtype == torch.float32 and new.residual.numel() == sum(s.numel() for s in shapes)
    assert [v.data_ptr() - new.residual.data_ptr() for v in new.views] == \
        [4 * sum(s.numel() for s in shapes[:i]) for i in range(len(shapes))]
    ref_flat = torch.zeros_like(new.residual)
    ref_views = _views(ref_flat, shapes)
    ref = PowerSGD(ref_views, cfg)
    assert torch.equal(ref._powersgd._ps_buffer, new.inner._powersgd._ps_buffer)
    assert new.is_compressed_mask == ref.is_compressed_mask
    if mcr == 2:
        assert any(new.is_compressed_mask) and not all(new.is_compressed_mask)
    oracles = []
    for _ in range(world):
        st = O.policy_init([torch.zeros(s) for s in SHAPES], rank, mcr, iters, start)
        st.codec.p_flat.copy_(ref._powersgd._ps_buffer.cpu())
        st.codec.q_flat.copy_(ref._powersgd._qs_buffer.cpu())
        oracles.append(st)
    ora_res = [[torch.zeros(s) for s in SHAPES] for _ in range(world)]
    ctx = (rank, iters, mcr, start, world, rank_id)
    for t in range(steps):
        fresh = [[g.to(BF16) for g in step_grads(t, w)] for w in range(world)]
        grads = [g.to(DEV) for g in fresh[rank_id]]
        for v, g in zip(ref_views, grads):
            v.add_(g.float())  # previous residual + fresh, one fp32 add
        out = new.aggregate(grads)
        ref_out = ref.aggregate(ref_views)
        torch.cuda.synchronize()
        assert new.step_counter == ref.step_counter == t + 1
        for i in range(len(shapes)):
            assert out[i].dtype == BF16 and out[i].shape == shapes[i]
            assert torch.equal(new.views[i], ref_views[i]), (ctx, t, i, "residual")
            assert torch.equal(_bits(out[i]), _bits(ref_out[i].to(BF16))), (ctx, t, i, "output")
            assert not bool(grads[i].view(torch.int16).any()), (ctx, t, i, "gradients are +0.0")
        # the oracle, free-running on the same upcast inputs
        gc = [[r + g.float() for r, g in zip(ora_res[w], fresh[w])] for w in range(world)]
        ins = [[x.clone() for x in gc[w]] for w in range(world)]
        want = MW.run_workers(oracles, gc)
        tol = TOL_STEP if t <= start else TOL_FREE
        for i in range(len(shapes)):
            scale = max((ins[w][i] for w in range(world)), key=lambda x: float(x.norm()))
            check(_rel(new.views[i], gc[rank_id][i], scale), tol, *ctx, t, i, "fp32res-residual")
            check(_rel(out[i].float(), want[rank_id][i], scale), TOL_BF16, *ctx, t, i, "fp32res-avg")
        ora_res = gc
    new.close()
    ref.close()


def _worker(rank_id, world, initfile, args):
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=world)
    try:
        _run(rank_id, world, *args)
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("rank,iters", [(2, 2), (1, 1), (4, 3)])
def test_matches_fp32_powersgd_bitwise(rank, iters):
    _run(0, 1, rank, iters, 2, 0, 3)


def test_warm_up_steps():
    _run(0, 1, 2, 2, 2, 2, 4)  # two all-reduce steps, then two compressed ones


@pytest.mark.parametrize("rank,iters", [(2, 2), (1, 1), (4, 3)])
def test_world_size_two(rank, iters):
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_worker, args=(2, os.path.join(td, "init"), (rank, iters, 2, 0, 3)), nprocs=2,
                                    join=True)


def test_optimizer_step_consumes_the_gradients():
    """``optimizer_step`` unchanged: p.grad is restored to the (zeroed) gradient tensors, the next
    backward accumulates fresh gradients only, and the residual carries the error."""
    from powersgd_amd import Config, Fp32ResidualPowerSGD, optimizer_step

    params = [torch.nn.Parameter(torch.zeros(s, dtype=BF16, device=DEV)) for s in SHAPES]
    opt = torch.optim.SGD(params, lr=1.0)
    agg = Fp32ResidualPowerSGD(params, Config(2, 2, 2, 0))
    seen = {}
    orig = agg.aggregate

    def spy(grads):
        seen["out"] = orig(grads)
        return seen["out"]

    agg.aggregate = spy
    for t in range(2):
        fresh = [g.to(BF16) for g in step_grads(t, 0)]
        for p, g in zip(params, fresh):
            if p.grad is None:
                p.grad = g.to(DEV)
            else:
                p.grad.add_(g.to(DEV))  # onto zeros: the fresh gradient alone
            assert torch.equal(p.grad.cpu(), g)
        held = [p.grad for p in params]
        before = [p.detach().clone() for p in params]
        optimizer_step(opt, agg)
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            assert p.grad.data_ptr() == held[i].data_ptr()  # the caller's gradient tensor, restored
            assert not bool(p.grad.view(torch.int16).any())  # ... consumed: +0.0 everywhere
            assert torch.equal(p.detach(), before[i] - seen["out"][i])  # SGD, lr 1, on the bf16 average
        assert agg.step_counter == t + 1 and bool(agg.residual.any())


def test_refuses_other_dtypes_and_bad_gradient_lists():
    from powersgd_amd import Config, Fp32ResidualPowerSGD

    cfg = Config(1, 2, 1, 0)
    for dt in (torch.float32, torch.float64):
        with pytest.raises(RuntimeError, match="use PowerSGD"):
            Fp32ResidualPowerSGD([torch.zeros(8, 4, dtype=dt, device=DEV)], cfg)
    with pytest.raises(IndexError):
        Fp32ResidualPowerSGD([], cfg)
    agg = Fp32ResidualPowerSGD([torch.zeros(8, 4, dtype=BF16, device=DEV), torch.zeros(3, dtype=BF16, device=DEV)], cfg)
    ok = [torch.ones(8, 4, dtype=BF16, device=DEV), torch.ones(3, dtype=BF16, device=DEV)]
    with pytest.raises(ValueError):
        agg.aggregate(ok[:1])
    with pytest.raises(RuntimeError, match="shape"):
        agg.aggregate([ok[0].view(4, 8), ok[1]])
    with pytest.raises(RuntimeError, match="scalar type"):
        agg.aggregate([ok[0].float(), ok[1]])
    with pytest.raises(RuntimeError):
        agg.aggregate([ok[0].cpu(), ok[1]])
    with pytest.raises(RuntimeError, match="contiguous"):
        agg.aggregate([torch.ones(4, 8, dtype=BF16, device=DEV).t(), ok[1]])
    torch.cuda.synchronize()
    assert agg.step_counter == 0 and not bool(agg.residual.any()) and bool((ok[0] == 1).all())  # nothing ran
