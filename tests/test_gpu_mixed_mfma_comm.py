"""psgd_aggregate_mixed_comm at rank buckets 16 and 32 (``Fp32ResidualPowerSGD(..., fused=True)`` in a
process group that runs over the library's own communicator: the matrix-core final pass of the
communicator sequence stores the bf16 averages) against the three-stage flow of the same build on
the same communicator (``fused=False``: run-table ADD, psgd_aggregate_comm on the fp32 residual,
run-table GATHER).

The fused call is defined as that sequence, so there is no tolerance: ``torch.equal`` on raw bits,
after every step, of the bf16 outputs, the fp32 residual and the codec's ``_ps_buffer`` /
``_qs_buffer``; the consumed gradients must be +0.0 everywhere, and two fused runs must agree.

World size 3 runs on ONE GPU through the stand-in collective library (tests/stubs/rccl_stub.hip,
set up as tests/test_gpu_mixed_comm.py does); x / 3 and alpha = float(1 / 3.0) are inexact, so a
multiply in place of the division, or a swapped term set, changes bits. A 1-rank communicator runs
the shared-term instance inside the communicator call.

Iterations: at W = 3 the final pass stages two term sets, so I = 1, 2 take the matrix-core tiles
(2 sets x 2 terms = 4 panels, the staging limit) and I = 3 (6 > 4) sends every tile to the VALU
fallback. The shape set and its branch classes are those of tests/test_gpu_mixed_mfma.py (which
asserts them from the pointers)."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (24, 136), (130, 67), (64, 3, 3, 3), (40,), (257, 260), (1, 96), (96, 1)]
STEPS = 4
CASES = [(rank, iters) for rank in (16, 32) for iters in (1, 2, 3)]


def _mcr(iters: int) -> float:
    # numel / (0.5 I min(rank, min(shape)) sum(shape)): of the shapes with both matrix dimensions
    # above 1 the smallest is (24, 136) at rank 32, 1.7 / I; (40,) is 2 / (16 I) at most
    return 1.5 / iters


def _fresh(t: int):
    """Seeded bf16 gradients of step t whose scale grows each step (non-trivial residuals); a few
    -0.0 among them (an fp32 add of -0.0 onto a +0.0 residual is +0.0: an add, not a copy)."""
    gen = torch.Generator().manual_seed(1000 + t)
    out = []
    for s in SHAPES:
        g = (torch.randn(s, generator=gen) * float(2 ** t)).to(BF16)
        g.view(-1)[::7] = -0.0
        out.append(g)
    return out


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


class _Child:
    """The child's side of a case: the stub as the library's collective library, a one-rank gloo
    group (it only makes is_distributed() true), one communicator of world `world`."""

    def __init__(self, init, world):
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
        self.world = world

    def aggregator(self, rank, iters, fused):
        from powersgd_amd import Config, Fp32ResidualPowerSGD, _lib

        agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=BF16, device=self.dev) for s in SHAPES],
                                   Config(rank, _mcr(iters), iters, 0), fused=fused)
        agg.inner._powersgd._comm = _lib.Comm(self.world, 0, _lib.comm_unique_id(), 0)
        mask = agg.is_compressed_mask
        for s, c in zip(SHAPES, mask):
            assert c or len(s) == 1 or 1 in s, (s, "both matrix dimensions above 1: compressed")
        assert not mask[SHAPES.index((40,))], mask
        return agg

    def flow(self, rank, iters, fused):
        """STEPS steps of one aggregator; per step the raw bits of everything observable."""
        agg = self.aggregator(rank, iters, fused)
        rec = []
        for t in range(STEPS):
            grads = [g.to(self.dev) for g in _fresh(t)]
            folds = agg.fused_folds()
            codec = agg.inner._powersgd
            plan_folds = codec._plan.mixed_folds_comm(codec.step_counter, self.world)
            out = agg.aggregate(grads)
            torch.cuda.synchronize()
            rec.append({
                "folds": folds,
                "plan_folds": plan_folds,
                "out": [_bits(o).cpu() for o in out],
                "residual": _bits(agg.residual).cpu(),
                "ps": _bits(codec._ps_buffer).cpu(),
                "qs": _bits(codec._qs_buffer).cpu(),
                "grads_zero": all(not bool(_bits(g).any()) for g in grads),
            })
            assert agg.step_counter == t + 1
        agg.close()
        return rec

    def close(self):
        torch.distributed.destroy_process_group()


def _same(a, b, ctx):
    for t, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x["out"], y["out"])):
            assert torch.equal(p, q), (ctx, t, i, "output")
        for k in ("residual", "ps", "qs"):
            assert torch.equal(x[k], y[k]), (ctx, t, k)
        assert x["grads_zero"] and y["grads_zero"], (ctx, t, "every gradient element is +0.0")


def _bitwise(_, init, world):
    ch = _Child(init, world)
    try:
        for rank, iters in CASES:
            ctx = (world, rank, iters)
            ref = ch.flow(rank, iters, False)  # the reference: computed once, never modified
            assert [r["folds"] for r in ref] == [(0, 0)] * STEPS, ctx  # fused=False never folds
            one = ch.flow(rank, iters, True)
            print(ctx, "folds", [r["folds"] for r in one], flush=True)
            _same(one, ref, ctx)
            two = ch.flow(rank, iters, True)
            _same(two, one, (ctx, "second fused run"))
            assert [r["plan_folds"] for r in one] == [(0, 1)] * STEPS, (ctx, [r["plan_folds"] for r in one])
            assert [r["folds"] for r in one] == [(0, 1)] * STEPS, (ctx, [r["folds"] for r in one])
            assert any(bool(r["residual"].any()) for r in one), ctx  # the residuals are non-trivial
    finally:
        ch.close()


def _init(tmp_path):
    return f"file://{tmp_path}/store"


def test_fused_equals_three_stage_flow_bitwise_world_3(tmp_path):
    """W = 3 through the stand-in: the two-term-set instance, ranks 16 / 32, I = 1, 2 on the matrix
    cores and I = 3 on the fallback."""
    torch.multiprocessing.spawn(_bitwise, args=(_init(tmp_path), 3), nprocs=1, join=True)


def test_fused_equals_three_stage_flow_bitwise_one_rank_communicator(tmp_path):
    """A communicator of world 1: the shared-term instance and the / 1 flat path inside the
    communicator call."""
    torch.multiprocessing.spawn(_bitwise, args=(_init(tmp_path), 1), nprocs=1, join=True)
