"""Global-norm clipping of the averages (psgd_clip_outputs, ``PowerSGD(max_grad_norm=...)``).

The norm comes from the low-rank factors (factor form: two Gram matrices per compressed matrix,
the n x m output is never read) or from the dense outputs (stream form). Checked here:
the stream form against the fp64 sum of squares on the CPU; the factor form against the stream
form and the fp64 norm of the returned outputs on the same step (every rank bucket, I = 1-4, both
step parities, a jointly normalised rank-1 group of three matrices scaled 1 / 4 / 7, where the
cross blocks between iterations do not vanish); the clip itself bit for bit; reproducibility;
warm-up steps and wide plans through the stream form; ``optimizer_step``; the fp32-residual
aggregator.

Tolerances. Stream form: N * 2^-53 for each of the two sums, 8e-12 at N = 70001, so 1e-10
relative. Factor form against the outputs: the project's per-step tolerance, 1e-5 * ||input|| for
fp32 and 1e-2 * ||input|| for bf16 outputs (the returned output may differ from the factors'
product by that much and no more).

Observed on an MI355X: |factors - outputs| / ||input|| at most 3.5e-10 (rank 1), 1.7e-9 (rank 2),
3.4e-9 (rank 4), 3.1e-10 (rank 8), 4.1e-6 (the bf16 case), 1.8e-09 (rank 16) and 1.4e-09 (rank 32).
The rank-16 / 32 cases on the [3, 200] matrix (n = r = 3) are the ones that found the plan giving
such a matrix the vector layout those buckets' kernels do not know (psgd_plan_create, base_vec):
before that fix they missed the bound by 8e-5 to 2.4e-3."""
import math

import pytest
import torch

from powersgd_amd import Config, Fp32ResidualPowerSGD, PowerSGD, _lib, optimizer_step

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INF = float("inf")
FACTORS, STREAM = _lib.Plan.NORM_FACTORS, _lib.Plan.NORM_STREAM
# the rank-1 joint-norm group (three matrices scaled 1, 4, 7), r capped by n, m % 4 != 0, a
# [256, 64] matrix (more than one row block per side at 256 rows), two 1-D (uncompressed) tensors
SHAPES = [(64, 32, 3, 3), (64, 32, 3, 3), (64, 32, 3, 3), (3, 200), (96, 201), (256, 64, 1, 1), (40,), (130,)]
SCALES = [1.0, 4.0, 7.0, 1.0, 1.0, 1.0, 1.0, 1.0]
RANK_ITERS = [(r, i) for r in (1, 2, 4, 8, 16, 32) for i in (1, 2, 3, 4) if i * r <= 64]


def _rate(shape, rank, iters):
    numel = math.prod(shape)
    return numel / (0.5 * iters * min(rank, min(shape)) * sum(shape))


def _config(rank, iters, start=0, shapes=SHAPES):
    """A min_compression_rate between the 1-D tensors' rates and the matrices': every matrix is
    compressed, every 1-D tensor is not."""
    lo = max(_rate(s, rank, iters) for s in shapes if len(s) == 1)
    hi = min(_rate(s, rank, iters) for s in shapes if len(s) > 1)
    assert lo < hi
    return Config(rank, math.sqrt(lo * hi), iters, start)


def _inputs(seed, dtype=torch.float32, shapes=SHAPES, scales=SCALES):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=gen) * k).to(dtype) for s, k in zip(shapes, scales)]


def _make(rank, iters, dtype=torch.float32, start=0, shapes=SHAPES, **kw):
    return PowerSGD([torch.zeros(s, device=DEV, dtype=dtype) for s in shapes], _config(rank, iters, start, shapes), **kw)


def _norm64(tensors):
    return math.sqrt(sum(float((t.double().cpu() ** 2).sum()) for t in tensors))


def _measure(psgd, form):
    """psgd_clip_outputs with max_norm = +inf on the step `psgd` just ran: (norm, coef) bits."""
    codec, u = psgd._powersgd, psgd._unc
    res = torch.full((2,), -1.0, dtype=torch.float64, device=DEV)
    codec._plan.clip_outputs(codec.step_counter - 1, 1, codec._slab.data_ptr(), u.slab.data_ptr() if u else 0,
                             u.numel if u else 0, INF, res.data_ptr(), torch.cuda.current_stream().cuda_stream, form)
    torch.cuda.synchronize()
    return res.cpu()


def _coef(max_norm, norm):
    return min(1.0, max_norm / (norm + 1e-6))


def _scaled(t, coef):
    c32 = torch.tensor(coef, dtype=torch.float64).to(torch.float32).to(t.device)
    if t.dtype == torch.float64:
        return t * coef
    return (t.float() * c32).to(t.dtype)


def _same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    itype = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(itype), b.contiguous().view(itype)))


# ------------------------------------------------------------------ 1. stream form
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_stream_form_matches_fp64_sum_of_squares(dtype):
    if dtype == torch.float64:
        torch.set_default_dtype(torch.float64)  # fp64 plans: P/Q follow the default dtype
    psgd = _make(2, 1, dtype)
    plan = psgd._powersgd._plan
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(11)
    for n in (1, 63, 4097, 70001):
        host = torch.randn(n + 1, generator=gen, dtype=torch.float64).to(dtype)
        buf = host.to(DEV)
        view = buf[1:]  # the base pointer offset by one element: a scalar head before the vectors
        assert view.data_ptr() % 16 != 0
        res = torch.zeros(2, dtype=torch.float64, device=DEV)
        plan.clip_outputs(0, 1, 0, view.data_ptr(), n, INF, res.data_ptr(), stream, STREAM)
        torch.cuda.synchronize()
        want = math.sqrt(float((host[1:].double() ** 2).sum()))
        got = float(res[0])
        print(f"stream {dtype} n={n}: rel err {abs(got - want) / want:.3e}")
        assert abs(got - want) <= 1e-10 * want, (dtype, n, got, want)
        assert float(res[1]) == 1.0
        assert torch.equal(buf.cpu(), host)  # +inf: nothing is scaled


# ------------------------------------------------------------------ 2. factor form
def _factor_case(rank, iters, dtype, tol):
    psgd = _make(rank, iters, dtype)
    plan = psgd._powersgd._plan
    grads = [torch.zeros(s, device=DEV, dtype=dtype) for s in SHAPES]
    worst = 0.0
    for step in range(2):  # both step parities
        new = _inputs(100 * rank + 10 * iters + step, dtype)
        for g, x in zip(grads, new):
            g += x.to(DEV)  # the residual of the previous step plus fresh gradients
        scale = _norm64(grads)
        outs = psgd.aggregate(grads)
        torch.cuda.synchronize()
        assert plan.norm_form(step, 1) == FACTORS, (rank, iters, step)  # no silent fall-back
        want = _norm64(outs)
        fac, stm = _measure(psgd, FACTORS), _measure(psgd, STREAM)
        print(f"factor rank={rank} I={iters} {dtype} step={step}: |factors - outputs| / ||input|| = "
              f"{abs(float(fac[0]) - want) / scale:.3e}, |factors - stream| / ||input|| = "
              f"{abs(float(fac[0]) - float(stm[0])) / scale:.3e}")
        assert abs(float(stm[0]) - want) <= 1e-10 * want
        assert abs(float(fac[0]) - want) <= tol * scale, (rank, iters, step, float(fac[0]), want)
        assert abs(float(fac[0]) - float(stm[0])) <= tol * scale, (rank, iters, step)
        assert float(fac[1]) == 1.0 and float(stm[1]) == 1.0
        worst = max(worst, abs(float(fac[0]) - want) / scale)
    return worst


@pytest.mark.parametrize("rank,iters", RANK_ITERS)
def test_factor_form_matches_stream_form_and_outputs(rank, iters):
    _factor_case(rank, iters, torch.float32, 1e-5)


def test_factor_form_bf16():
    _factor_case(4, 2, torch.bfloat16, 1e-2)


def test_factor_form_refusals():
    psgd = _make(4, 2)
    plan, codec = psgd._powersgd._plan, psgd._powersgd
    res = torch.zeros(2, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert plan.norm_form(0, 1) == STREAM  # bound, no step has run: no record
    with pytest.raises(RuntimeError, match="no record"):  # refused before anything reads `out`
        plan.clip_outputs(0, 1, res.data_ptr(), 0, 0, INF, res.data_ptr(), stream, FACTORS)
    outs = psgd.aggregate([g.to(DEV) for g in _inputs(5)])
    args = (codec._slab.data_ptr(), psgd._unc.slab.data_ptr(), psgd._unc.numel)
    assert outs[0].data_ptr() == args[0]
    plan.clip_outputs(0, 1, *args, INF, res.data_ptr(), stream, FACTORS)
    for step, world in ((1, 1), (0, 2)):  # another step, another world size: stale
        assert plan.norm_form(step, world) == STREAM
        with pytest.raises(RuntimeError, match="no record"):
            plan.clip_outputs(step, world, *args, INF, res.data_ptr(), stream, FACTORS)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            plan.clip_outputs(0, 1, *args, bad, res.data_ptr(), stream, 0)
    wide = _make(64, 1, shapes=WIDE_SHAPES)
    wide.aggregate([g.to(DEV) for g in _inputs(6, shapes=WIDE_SHAPES, scales=[1.0] * len(WIDE_SHAPES))])
    with pytest.raises(ValueError, match="factor form"):
        wide._powersgd._plan.clip_outputs(0, 1, wide._powersgd._slab.data_ptr(), 0, 0, INF, res.data_ptr(), stream,
                                          FACTORS)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. clipping, bit for bit
@pytest.mark.parametrize("dtype,rank,iters", [(torch.float32, 1, 2), (torch.float32, 4, 1), (torch.bfloat16, 2, 2)])
def test_clip_scales_outputs_bitwise_and_leaves_residual(dtype, rank, iters):
    twin = _make(rank, iters, dtype)
    probe = _make(rank, iters, dtype, max_grad_norm=INF)
    for step in range(2):
        new = _inputs(40 + step, dtype)
        g_twin = [x.to(DEV) for x in new]
        before = [o.clone() for o in twin.aggregate(g_twin)]
        probe.aggregate([x.to(DEV) for x in new])
        norm = float(probe.last_grad_norm)
        assert abs(norm - _norm64(before)) <= (1e-2 if dtype == torch.bfloat16 else 1e-5) * _norm64(new)
        assert float(probe.last_clip_coef) == 1.0
        if step == 0:
            half, double = _make(rank, iters, dtype, max_grad_norm=norm / 2), _make(rank, iters, dtype, max_grad_norm=1.0)
        half.max_grad_norm, double.max_grad_norm = norm / 2, norm * 2  # the attribute is settable
        g_half, g_double = [x.to(DEV) for x in new], [x.to(DEV) for x in new]
        o_half, o_double = half.aggregate(g_half), double.aggregate(g_double)
        torch.cuda.synchronize()
        assert half._powersgd._plan.norm_form(step, 1) == FACTORS
        assert float(half.last_grad_norm) == norm  # the same inputs: the same bits
        coef = _coef(norm / 2, float(half.last_grad_norm))
        assert coef < 1.0 and float(half.last_clip_coef) == coef
        for a, b in zip(o_half, before):
            assert _same_bits(a, _scaled(b, coef))
        assert float(double.last_clip_coef) == 1.0
        for a, b in zip(o_double, before):
            assert _same_bits(a, b)
        for r_half, r_double, r_twin in zip(g_half, g_double, g_twin):  # clipping never touches the residual
            assert _same_bits(r_half, r_twin) and _same_bits(r_double, r_twin)


# ------------------------------------------------------------------ 4. reproducibility
def test_two_runs_give_identical_norm_bits():
    bits = []
    for _ in range(2):
        psgd = _make(4, 2)
        psgd.aggregate([x.to(DEV) for x in _inputs(77)])
        bits.append((_measure(psgd, FACTORS), _measure(psgd, STREAM), _measure(psgd, FACTORS)))
    for k in range(3):
        assert _same_bits(bits[0][k], bits[1][k])
    assert _same_bits(bits[0][0], bits[0][2])


# ------------------------------------------------------------------ 5. warm-up, wide plans, inf
WIDE_SHAPES = [(96, 201), (256, 64, 1, 1), (40,), (130,)]


def _clip_against_twin(make, inputs, steps, expect_form):
    twin, probe = make(), make(max_grad_norm=INF)
    clipped = None
    for step in range(steps):
        new = inputs(step)
        before = [o.clone() for o in twin.aggregate([x.to(DEV) for x in new])]
        probe.aggregate([x.to(DEV) for x in new])
        norm = float(probe.last_grad_norm)
        want = _norm64(before)
        assert abs(norm - want) <= 1e-10 * want  # the stream form
        if clipped is None:
            clipped = make(max_grad_norm=norm / 2)
        clipped.max_grad_norm = norm / 2
        outs = clipped.aggregate([x.to(DEV) for x in new])
        torch.cuda.synchronize()
        if expect_form is not None:
            assert clipped._powersgd._plan.norm_form(clipped._powersgd.step_counter - 1, 1) == expect_form
        coef = _coef(norm / 2, float(clipped.last_grad_norm))
        assert float(clipped.last_clip_coef) == coef and coef < 1.0
        for a, b in zip(outs, before):
            assert _same_bits(a, _scaled(b, coef))


def test_warm_up_step_clips_through_the_stream_form():
    """start_compressing_after_num_steps = 1: step 0 returns the AllReduce slab (every tensor
    uncompressed), step 1 compresses."""
    _clip_against_twin(lambda **kw: _make(2, 2, start=1, **kw), lambda t: _inputs(300 + t), 1, None)


def test_wide_plan_clips_through_the_stream_form():
    ones = [1.0] * len(WIDE_SHAPES)
    _clip_against_twin(lambda **kw: _make(64, 1, shapes=WIDE_SHAPES, **kw),
                       lambda t: _inputs(310 + t, shapes=WIDE_SHAPES, scales=ones), 2, STREAM)


def test_inf_in_the_flat_slab_leaves_outputs_untouched():
    new = _inputs(320)
    new[-1][7] = INF  # an uncompressed (1-D) tensor
    twin, clipped = _make(4, 2), _make(4, 2, max_grad_norm=1e-3)
    before = twin.aggregate([x.to(DEV) for x in new])
    outs = clipped.aggregate([x.to(DEV) for x in new])
    torch.cuda.synchronize()
    assert math.isinf(float(clipped.last_grad_norm)) and math.isnan(float(clipped.last_clip_coef))
    for a, b in zip(outs, before):
        assert _same_bits(a, b)


# ------------------------------------------------------------------ 6. optimizer_step
def test_optimizer_step_updates_with_the_clipped_average():
    new = _inputs(330)
    twin = _make(4, 2)
    g_twin = [x.to(DEV) for x in new]
    avg = twin.aggregate(g_twin)
    params = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in SHAPES]
    for p, x in zip(params, new):
        p.grad = x.to(DEV)
    agg = PowerSGD(params, _config(4, 2), max_grad_norm=_norm64(avg) / 2)
    opt = torch.optim.SGD(params, lr=1.0)
    optimizer_step(opt, agg)
    torch.cuda.synchronize()
    coef = _coef(agg.max_grad_norm, float(agg.last_grad_norm))
    assert coef < 1.0 and float(agg.last_clip_coef) == coef
    for p, a, r in zip(params, avg, g_twin):
        assert torch.equal(p.data, -_scaled(a, coef))  # lr 1, no momentum, from zero: minus the clipped average
        assert _same_bits(p.grad, r)                  # the unclipped twin's residual


# ------------------------------------------------------------------ 7. fp32 residual of bf16 gradients
def test_fp32_residual_clips_before_the_bf16_rounding():
    cfg = _config(4, 2)
    params = [torch.zeros(s, device=DEV, dtype=torch.bfloat16) for s in SHAPES]
    plain = Fp32ResidualPowerSGD(params, cfg, fused=True)
    assert plain.fused_folds()[1] == 1  # without a value the fused path still reports its folds
    assert plain.max_grad_norm is None
    twin = Fp32ResidualPowerSGD(params, cfg)  # its fp32 stage run by hand: ADD, the fp32 codec
    clipped = None
    for step in range(2):
        new = _inputs(340 + step, torch.bfloat16)
        for v, x in zip(twin.views, new):
            v += x.to(DEV).float()
        avg = [a.clone() for a in twin.inner.aggregate(twin.views)]
        x = _norm64(avg) / 2
        if clipped is None:
            clipped = Fp32ResidualPowerSGD(params, cfg, fused=True, max_grad_norm=x)
        clipped.max_grad_norm = x
        assert clipped.fused_folds() == (0, 0)
        grads = [g.to(DEV) for g in new]
        outs = clipped.aggregate(grads)
        torch.cuda.synchronize()
        coef = _coef(x, float(clipped.last_grad_norm))
        assert coef < 1.0 and float(clipped.last_clip_coef) == coef
        for o, a in zip(outs, avg):
            assert o.dtype == torch.bfloat16
            assert _same_bits(o, (a * torch.tensor(coef, dtype=torch.float64).to(torch.float32).to(DEV)).to(torch.bfloat16))
        for g in grads:
            assert not bool(g.any())  # consumed
        for v, w in zip(clipped.views, twin.views):
            assert _same_bits(v, w)  # the residual is the unclipped twin's
