"""``Fp32ResidualPowerSGD(..., fused=True)`` at rank buckets 16 and 32 (psgd_aggregate_mixed with the
matrix-core final pass storing the bf16 averages) against the three-stage flow of the same build
(``fused=False``: run-table ADD, fp32 codec, run-table GATHER).

The fused call is defined as that sequence, so there is no tolerance: every comparison is
``torch.equal`` on raw bits, after every step, of the bf16 outputs, the fp32 residual and the
codec's ``_ps_buffer`` / ``_qs_buffer``; the consumed gradients must be +0.0 everywhere, and two
fused runs must agree bit for bit.

The shapes (fp32 residual views back to back, in this order) make every branch of the final pass
occur; ``test_shape_classes`` asserts each class from the pointers and shapes:

* matrix-core tiles with n % 16 != 0 and m % 64 != 0: (300, 520), twice (a two-matrix group);
* a matrix-core matrix whose effective rank is below the bucket: (24, 136) at rank 32, and every
  matrix at ranks 12 / 24;
* the VALU fallback by m % 4 != 0: (130, 67) and (64, 27);
* the VALU fallback by alignment alone: (257, 260), whose residual view and output offset are 8-byte
  aligned only;
* uncompressed tensors (the flat tail): at least (40,).

At I = 5 (rank 16) the terms exceed the staged panels and every tile takes the fallback."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (24, 136), (130, 67), (64, 3, 3, 3), (40,), (257, 260), (1, 96), (96, 1)]
STEPS = 4
CASES = [(r, i) for r in (12, 16, 24, 32) for i in (1, 2, 3, 4)] + [(16, 5)]


def _mcr(iters: int) -> float:
    # numel / (0.5 I min(rank, min(shape)) sum(shape)): of the shapes with both matrix dimensions
    # above 1 the smallest is (24, 136) at ranks >= 24, 1.7 / I; (40,) is at most 2 / (12 I)
    return 1.5 / iters


def _matrix(shape):
    return (shape[0], int(torch.Size(shape[1:]).numel())) if len(shape) > 1 else (shape[0], 1)


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


def _aggregator(rank: int, iters: int, fused: bool):
    from powersgd_amd import Config, Fp32ResidualPowerSGD

    cfg = Config(rank, _mcr(iters), iters, 0)
    agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=BF16, device=DEV) for s in SHAPES], cfg, fused=fused)
    mask = agg.is_compressed_mask
    for s, c in zip(SHAPES, mask):
        n, m = _matrix(s)
        assert c or not (n > 1 and m > 1), (s, "both matrix dimensions above 1: compressed")
    assert not mask[SHAPES.index((40,))], mask
    return agg


def _flow(rank: int, iters: int, odd: bool, fused: bool):
    """STEPS steps of one aggregator; per step the raw bits of everything observable."""
    agg = _aggregator(rank, iters, fused)
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
def _unfused(rank: int, iters: int, odd: bool):
    return _flow(rank, iters, odd, False)  # the reference: computed once, never modified


def _same(a, b, ctx):
    for t, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x["out"], y["out"])):
            assert torch.equal(p, q), (ctx, t, i, "output")
        for k in ("residual", "ps", "qs"):
            assert torch.equal(x[k], y[k]), (ctx, t, k)
        assert x["grads_zero"] and y["grads_zero"], (ctx, t, "every gradient element is +0.0")


def _compare(rank, iters, odd):
    ctx = (rank, iters, odd)
    ref = _unfused(rank, iters, odd)
    assert [r["folds"] for r in ref] == [(0, 0)] * STEPS  # fused=False never folds
    one = _flow(rank, iters, odd, True)
    for t, r in enumerate(one):
        print(ctx, "step", t, "folds", r["folds"])
    _same(one, ref, ctx)
    two = _flow(rank, iters, odd, True)
    _same(two, one, (ctx, "second fused run"))
    # the output fold on every step; no ingest fold at these ranks (no single-pass final kernel)
    assert [r["folds"] for r in one] == [(0, 1)] * STEPS, ctx
    assert any(bool(r["residual"].any()) for r in one)  # the residuals are non-trivial


@pytest.mark.parametrize("rank,iters", CASES)
def test_fused_equals_three_stage_flow_bitwise(rank, iters):
    _compare(rank, iters, False)


@pytest.mark.parametrize("rank", [12, 16, 24, 32])
def test_fused_equals_three_stage_flow_bitwise_odd_offset_views(rank):
    _compare(rank, 2, True)


@pytest.mark.parametrize("rank", [16, 32])
def test_shape_classes(rank):
    """The branches the shape set is chosen for, from the residual views' pointers, the plan's
    output offsets and the shapes: what k_apply<float> and the mixed kernels both test."""
    agg = _aggregator(rank, 2, True)
    plan = agg.inner._powersgd._plan
    comp = [i for i, c in enumerate(agg.is_compressed_mask) if c]
    offs = dict(zip(comp, plan.output_offsets()))
    cls = {}
    for i in comp:
        n, m = _matrix(SHAPES[i])
        al = agg.views[i].data_ptr() % 16 == 0 and (offs[i] * 4) % 16 == 0
        cls[i] = "m%4" if m % 4 else "matrix-core" if al else "alignment"
    idx = {s: [i for i, x in enumerate(SHAPES) if x == s] for s in set(SHAPES)}
    assert [cls[i] for i in idx[(300, 520)]] == ["matrix-core"] * 2
    assert 300 % 16 and 520 % 64
    assert cls[idx[(24, 136)][0]] == "matrix-core" and (rank < 32 or min(24, 136) < rank)
    assert cls[idx[(130, 67)][0]] == "m%4" and cls[idx[(64, 3, 3, 3)][0]] == "m%4"
    i = idx[(257, 260)][0]
    assert cls[i] == "alignment" and agg.views[i].data_ptr() % 16 == 8 and (offs[i] * 4) % 16 == 8
    assert not agg.is_compressed_mask[idx[(40,)][0]]
    agg.close()


def test_direct_call_on_a_rank_16_plan_equals_the_sequence():
    """psgd_aggregate_mixed called directly on a rank-16 plan: served (no ValueError), folds
    (0, 1), and bit for bit the ADD, psgd_aggregate on the residual and the bf16 rounding."""
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    shapes = [(300, 520), (130, 67), (257, 260)]
    numel = [torch.Size(s).numel() for s in shapes]

    def run(direct: bool):
        codec = BasicPowerSGD([torch.zeros(s, device=DEV) for s in shapes], BasicConfig(16, 2))
        assert codec._plan.mixed_folds(0) == (0, 1) and codec._plan.mixed_folds(1) == (0, 1)
        gen = torch.Generator().manual_seed(5)
        grads = [torch.randn(s, generator=gen).to(BF16).to(DEV) for s in shapes]
        resid = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
        if direct:
            out = torch.full((sum(numel),), 3.0, dtype=BF16, device=DEV)
            gp = _lib.ptr_array([g.data_ptr() for g in grads])
            rp = _lib.ptr_array([r.data_ptr() for r in resid])
            codec._plan.aggregate_mixed(ctypes.addressof(gp), ctypes.addressof(rp), out.data_ptr(), 0,
                                        torch.cuda.current_stream(DEV).cuda_stream)
            torch.cuda.synchronize()
            assert all(not bool(_bits(g).any()) for g in grads)  # consumed: +0.0 everywhere
        else:
            for r, g in zip(resid, grads):
                r += g.float()
                g.zero_()
            out = torch.cat([o.reshape(-1) for o in codec.aggregate(resid)]).to(BF16)
        torch.cuda.synchronize()
        return [_bits(out).cpu()] + [_bits(r).cpu() for r in resid] + [_bits(codec._ps_buffer).cpu(),
                                                                        _bits(codec._qs_buffer).cpu()]

    for x, y in zip(run(True), run(False)):
        assert torch.equal(x, y)
