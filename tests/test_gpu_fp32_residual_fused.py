"""``Fp32ResidualPowerSGD(..., fused=True)`` (psgd_aggregate_mixed: the bf16 averages stored by
the codec's final pass, the bf16 gradients ingested by the single-pass final kernel or by an ADD
the library launches) against the
three-stage flow of the same build (``fused=False``: run-table ADD, fp32 codec, run-table GATHER).

The fused call is defined as that sequence, so there is no tolerance: every comparison is
``torch.equal`` on raw bits, after every step, of the bf16 outputs, the fp32 residual and the
codec's ``_ps_buffer`` / ``_qs_buffer``; the consumed gradients must be +0.0 everywhere, and two
fused runs must agree bit for bit.

Shapes: a two-matrix shape group (the rank-1 joint norm), m % 4 != 0, more than 256 rows and more
than 256 columns, a 1-D tensor and the degenerate panels (1, m) / (n, 1); every case also with the
bf16 gradients as views at odd element offsets of one flat buffer (2-byte aligned only: the
element-access paths). ``min_compression_rate`` leaves at least one tensor uncompressed: at rank 1
the degenerate panels (the 1-D tensor is then a compressed [40, 1] matrix), above it the 1-D
tensor (and the degenerate panels are compressed)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3), (40,), (257, 260), (1, 96), (96, 1)]
STEPS = 4


def _mcr(rank: int, iters: int) -> float:
    # numel / (0.5 I r sum(shape)): (40,) is 2 / (I r), (1, 96) and (96, 1) are 1.979 / I
    return (1.99 if rank == 1 else 1.5) / iters


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


def _place(fresh, odd: bool):
    """The step's gradients on the device: separate tensors, or views at odd element offsets of
    one flat bf16 buffer (whose base is 4-byte aligned or better: every view is 2-byte aligned only)."""
    if not odd:
        return [g.to(DEV) for g in fresh]
    total = sum(g.numel() + 2 for g in fresh) + 1
    flat = torch.zeros(total, dtype=BF16, device=DEV)
    views, off = [], 1
    for g in fresh:
        v = flat[off:off + g.numel()].view(g.shape)
        assert v.data_ptr() % 4 == 2
        v.copy_(g)
        views.append(v)
        off += g.numel() + (2 if g.numel() % 2 == 0 else 1)
    return views


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


def _flow(rank: int, iters: int, odd: bool, fused: bool, start: int = 0, mcr=None):
    """STEPS steps of one aggregator; per step the raw bits of everything observable."""
    from powersgd_amd import Config, Fp32ResidualPowerSGD

    cfg = Config(rank, _mcr(rank, iters) if mcr is None else mcr, iters, start)
    agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=BF16, device=DEV) for s in SHAPES], cfg, fused=fused)
    mask = agg.is_compressed_mask
    assert any(mask) and not all(mask), mask
    rec = []
    for t in range(STEPS):
        grads = _place(_fresh(t), odd)
        folds = agg.fused_folds()
        out = agg.aggregate(grads)
        torch.cuda.synchronize()
        codec = agg.inner._powersgd
        rec.append({
            "folds": folds,
            "out": [_bits(o).cpu() for o in out],
            "residual": _bits(agg.residual).cpu(),
            "ps": _bits(codec._ps_buffer).cpu(),
            "qs": _bits(codec._qs_buffer).cpu(),
            "grads_zero": all(not bool(_bits(g).any()) for g in grads),
        })
        assert agg.step_counter == t + 1
    agg.close()
    return rec


@functools.lru_cache(maxsize=None)
def _unfused(rank: int, iters: int, odd: bool, start: int = 0, mcr=None):
    return _flow(rank, iters, odd, False, start, mcr)  # the reference: computed once, never modified


def _same(a, b, ctx):
    for t, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x["out"], y["out"])):
            assert torch.equal(p, q), (ctx, t, i, "output")
        for k in ("residual", "ps", "qs"):
            assert torch.equal(x[k], y[k]), (ctx, t, k)
        assert x["grads_zero"] and y["grads_zero"], (ctx, t, "every gradient element is +0.0")


# (fold_in, fold_out) by step parity (steps 0, 1, 2, 3). The output fold is on every step. The
# ingest fold lives in the single-pass final kernel alone: I = 1 on odd steps, at ranks 1 and 2 (the
# K-term form is not built for rank 4, whose odd steps start in the unfused odd product). Steps
# that start in k_even report 0: that fold was built, measured slower than the run-table ADD it
# replaces (cfg4 even steps 0.2618 against 0.2559 ms, ResNet-50 0.1265 against 0.1222 ms, DESIGN
# section 10) and, by the rule that a slower fold is never kept, dropped; the library launches the
# ADD there, as it does where the first pass is the odd-even pass or the unfused odd product.
FOLDS = {
    1: [(0, 1), (1, 1), (0, 1), (1, 1)],
    2: [(0, 1), (0, 1), (0, 1), (0, 1)],
    3: [(0, 1), (0, 1), (0, 1), (0, 1)],
}


def _folds(rank: int, iters: int):
    if rank == 4 and iters == 1:
        return [(0, 1)] * STEPS
    return FOLDS[iters]


@pytest.mark.parametrize("odd", [False, True], ids=["separate", "odd-offset-views"])
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("rank", [1, 2, 4])
def test_fused_equals_three_stage_flow_bitwise(rank, iters, odd):
    ctx = (rank, iters, odd)
    ref = _unfused(rank, iters, odd)
    assert [r["folds"] for r in ref] == [(0, 0)] * STEPS  # fused=False never folds
    one = _flow(rank, iters, odd, True)
    for t, r in enumerate(one):
        print(ctx, "step", t, "folds", r["folds"])
    _same(one, ref, ctx)
    two = _flow(rank, iters, odd, True)
    _same(two, one, (ctx, "second fused run"))
    assert [r["folds"] for r in one] == _folds(rank, iters), ctx
    assert any(bool(r["residual"].any()) for r in one)  # the residuals are non-trivial


def test_rank_8_falls_back():
    """Rank bucket 8 has no mixed instances: 0 / 0, and fused=True runs the three-stage flow."""
    ref = _unfused(8, 2, False, 0, 0.3)
    got = _flow(8, 2, False, True, 0, 0.3)
    assert [r["folds"] for r in got] == [(0, 0)] * STEPS
    _same(got, ref, "rank 8")


def test_warm_up_steps_fall_back():
    """start_compressing_after_num_steps = 2: the two all-reduce steps report 0 / 0 and run the
    three-stage flow, the compressed ones after them fold."""
    ref = _unfused(2, 2, False, 2)
    got = _flow(2, 2, False, True, 2)
    assert [r["folds"] for r in got] == [(0, 0), (0, 0), (0, 1), (0, 1)]
    _same(got, ref, "warm-up")


@pytest.mark.parametrize("what", ["rank8", "bf16", "wide"])
def test_direct_call_refuses_other_plans_and_touches_nothing(what):
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    shapes = [(300, 520), (130, 67)]
    rank = {"rank8": 8, "bf16": 2, "wide": 64}[what]
    dt = BF16 if what == "bf16" else torch.float32
    codec = BasicPowerSGD([torch.zeros(s, dtype=dt, device=DEV) for s in shapes], BasicConfig(rank, 2))
    assert codec._plan.is_wide() == (what == "wide")
    assert codec._plan.mixed_folds(0) == (0, 0) and codec._plan.mixed_folds(1) == (0, 0)
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(s, generator=gen).to(BF16).to(DEV) for s in shapes]
    resid = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
    out = torch.full((sum(torch.Size(s).numel() for s in shapes),), 3.0, dtype=BF16, device=DEV)
    keep = [x.clone() for x in grads + resid + [out, codec._ps_buffer, codec._qs_buffer]]
    gp = _lib.ptr_array([g.data_ptr() for g in grads])
    rp = _lib.ptr_array([r.data_ptr() for r in resid])
    with pytest.raises(ValueError, match="psgd_aggregate_mixed"):
        codec._plan.aggregate_mixed(ctypes.addressof(gp), ctypes.addressof(rp), out.data_ptr(), 0,
                                    torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    for a, b in zip(grads + resid + [out, codec._ps_buffer, codec._qs_buffer], keep):
        assert torch.equal(_bits(a) if a.dtype == BF16 else a, _bits(b) if b.dtype == BF16 else b)
