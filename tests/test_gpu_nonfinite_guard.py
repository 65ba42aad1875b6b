"""``skip_nonfinite=True``: a step whose aggregates are not finite is skipped on the device
(psgd_guard_outputs: k_guard_check scans the P / Q state and the dense uncompressed slab,
k_guard_apply zeroes averages and gradients and puts P / Q back to ``reset_p`` / ``reset_q``).

The shapes are those of tests/test_gpu_clip.py: a rank-1 joint group of three matrices, [3, 200]
(r capped by n), [96, 201] (m % 4 != 0), [256, 64, 1, 1] and two 1-D (uncompressed) tensors.

Checked here: finite steps are bitwise the unguarded run's; a poisoned step returns all-zero bits,
leaves all-zero gradients and P / Q equal to the reset copies, and every other step matches the CPU
oracle from an identical state (a FRESH ``policy_init`` with the device's two step counters right
after the skip); warm-up steps; the scan's edges (head / vectors / tail of a misaligned slab, every
slab dtype, the first and last element of P and Q); the zeroing stores' bounds through sentinels
between misaligned gradient views; ``max_grad_norm``; ``Fp32ResidualPowerSGD``; ``optimizer_step``;
the DDP hook; world size 3 through the stand-in communicator.

Tolerances are the project's per-step ones from an identical state (DESIGN.md section 5,
tests/test_gpu_parity.py): ||ours - oracle||_F <= TOL * ||input||_F per tensor, TOL = 1e-5 (fp32),
1e-12 (fp64), 4e-3 (bf16 gradients, the oracle on the bf16-rounded inputs). After every compared
step the oracle takes the device's P / Q (as tests/test_gpu_capped_rank.py does), so each step
starts from an identical state; the step right after a skip starts from the fresh oracle as it is.
Everything else is bit for bit.

Well-posedness (as tests/test_gpu_capped_rank.py). Where iters * r exceeds min(n, m) of a matrix,
the state a step leaves has columns that are pure rounding, and the NEXT step's orthonormalisation
of that state is decided by them: the reference itself is then not defined to the bound. The test
measures this on the CPU alone, on every compared step: the oracle in fp32 and in float64 from the
same state and inputs; where the two differ by more than a tenth of the bound for a tensor, the
oracle cannot arbitrate that tensor-case and it keeps the error-feedback identity (||out + residual
- input|| <= 1e-6 ||input||) instead. That never happens on a step from a fresh state (asserted: the
first step and the step right after a skip are always held against the oracle), and every later
step after a skip, gated or not, is ALSO held bit for bit (outputs, residual, P, Q) against a
freshly constructed, unguarded aggregator with the same counters and seed, which is the claim
itself: after a skipped step the codec is a fresh one except for its counters.
Gated on an MI355X run, all at step 3 with the skip at step 1 (the second step from the fresh
state): (rank 2, I 2) the [3, 200] matrix (2 * 2 > 3; device against oracle 9.9e-3, the oracle's
fp32 against its float64 2.6e-3) and (rank 40, I 2) the three [64, 288] matrices (2 * 40 > 64;
0.18 - 0.21 against 0.15 - 0.19). Nothing is gated at world size 3 (rank 4, I 2) or in bf16.

Observed on an MI355X, over all compared tensor-cases: fp32 at most 5.6e-7 (bound 1e-5), world
size 3 1.5e-7, bf16 outputs 4.7e-4 and residuals 1.6e-3 (4e-3), fp64 3.2e-16 (1e-12), the error
feedback of the gated cases 1.3e-8 (1e-6)."""
import math
import os

import pytest
import torch

from oracle import powersgd_oracle as O
from parity_log import check
from powersgd_amd import Config, Fp32ResidualPowerSGD, PowerSGD, _lib, optimizer_step
from test_gpu_clip import SHAPES, _config, _inputs, _make, _same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN, INF = float("nan"), float("inf")
TOL = {torch.float32: 1e-5, torch.float64: 1e-12, torch.bfloat16: 4e-3}
# error feedback, out + residual = input: 1e-6 (1e-12 in fp64); bf16 stores round at 2^-9 each: 2.8e-3 < 4e-3
TOL_EF = {torch.float32: 1e-6, torch.float64: 1e-12, torch.bfloat16: 4e-3}
RANK_ITERS = [(1, 1), (1, 2), (2, 2), (4, 3), (8, 2), (16, 2), (32, 1), (40, 2)]
LAST_COMPRESSED = 5  # [256, 64, 1, 1]
POISONS = {
    "nan-joint": (1, 777, NAN),               # one element of a joint-group matrix
    "pinf-96x201": (4, 50 * 201 + 100, INF),  # the m % 4 != 0 matrix
    "ninf-1d": (6, 7, -INF),                  # an uncompressed tensor
    "nan-last": (LAST_COMPRESSED, -1, NAN),   # the last element of the last compressed tensor
}


def _poison(grads, kind):
    i, at, value = POISONS[kind]
    grads[i].view(-1)[at] = value


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _all_zero_bits(t):
    itype = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return not bool(t.contiguous().view(itype).any())


def _rel(a, b, scale):
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(float(scale.double().norm()), 1e-300)


def _flags(agg):
    return int(agg.last_step_skipped), int(agg.skipped_steps)


def _oracle(rank, iters, start=0):
    cfg = _config(rank, iters, start)
    return O.policy_init([torch.zeros(s) for s in SHAPES], rank, cfg.min_compression_rate, iters, start)


def _seed_from_oracle(psgd, ora):
    """The oracle's initial P / Q into the state and into the reset copies."""
    codec = psgd._powersgd
    for dst in (codec._ps_buffer, psgd.reset_p):
        dst.copy_(ora.codec.p_flat.to(dst.dtype))
    for dst in (codec._qs_buffer, psgd.reset_q):
        dst.copy_(ora.codec.q_flat.to(dst.dtype))


def _sync_oracle(ora, psgd):
    ora.codec.p_flat.copy_(psgd._powersgd._ps_buffer.cpu())
    ora.codec.q_flat.copy_(psgd._powersgd._qs_buffer.cpu())


def _fresh_oracle_like(psgd, rank, iters, start=0):
    """A fresh ``policy_init`` whose two step counters are the device's."""
    ora = _oracle(rank, iters, start)
    ora.step, ora.codec.step = psgd.step_counter, psgd._powersgd.step_counter
    return ora


def _oracle_inputs(gd):
    # the oracle sees exactly the device inputs (bf16: rounded, upcast)
    return [(g.float() if g.dtype == torch.bfloat16 else g).cpu().clone() for g in gd]


def _oracle64(ora, rank, iters, start=0):
    """`ora` (an fp32 oracle state, before a step) restated in float64: same P / Q values and counters."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        wide = _oracle(rank, iters, start)
    finally:
        torch.set_default_dtype(prev)
    wide.codec.p_flat.copy_(ora.codec.p_flat)
    wide.codec.q_flat.copy_(ora.codec.q_flat)
    wide.step, wide.codec.step = ora.step, ora.codec.step
    return wide


def _own_error(want, res, want64, res64, scales):
    """Per tensor, the reference's own error on this step: fp32 oracle against float64 oracle from
    the same state and inputs, outputs and residuals, relative to ||input||."""
    return [max(_rel(w, w64, s), _rel(r, r64, s)) for w, r, w64, r64, s in zip(want, res, want64, res64, scales)]


def _twin(psgd, ora0, rank, iters, dtype, start):
    """A freshly constructed, unguarded aggregator with `psgd`'s two counters and the same seed."""
    twin = _make(rank, iters, dtype, start)
    twin._powersgd._ps_buffer.copy_(ora0[0].to(twin._powersgd._ps_buffer.dtype))
    twin._powersgd._qs_buffer.copy_(ora0[1].to(twin._powersgd._qs_buffer.dtype))
    twin.step_counter, twin._powersgd.step_counter = psgd.step_counter, psgd._powersgd.step_counter
    return twin


# ------------------------------------------------------------------ 1. finite steps are untouched
def _finite_case(rank, iters, dtype):
    if dtype == torch.float64:
        torch.set_default_dtype(torch.float64)  # fp64 plans: P/Q follow the default dtype
    on, off = _make(rank, iters, dtype, skip_nonfinite=True), _make(rank, iters, dtype)
    assert on.skip_nonfinite is True and off.skip_nonfinite is False
    assert off.last_step_skipped is None and off.skipped_steps is None and off.reset_p is None
    for t in (on.last_step_skipped, on.skipped_steps):
        assert t.dim() == 0 and t.dtype == torch.int64 and t.is_cuda
    assert on.last_step_skipped.untyped_storage().data_ptr() == on.skipped_steps.untyped_storage().data_ptr()
    assert _same_bits(on.reset_p, on._powersgd._ps_buffer) and _same_bits(on.reset_q, on._powersgd._qs_buffer)
    assert on.reset_p.data_ptr() != on._powersgd._ps_buffer.data_ptr()
    g_on = [torch.zeros(s, device=DEV, dtype=dtype) for s in SHAPES]
    g_off = [torch.zeros(s, device=DEV, dtype=dtype) for s in SHAPES]
    for step in range(3):
        for a, b, x in zip(g_on, g_off, _inputs(900 + 10 * rank + step, dtype)):
            a += x.to(DEV)
            b += x.to(DEV)
        o_on, o_off = on.aggregate(g_on), off.aggregate(g_off)
        torch.cuda.synchronize()
        for a, b in zip(o_on + g_on, o_off + g_off):
            assert _same_bits(a, b), (rank, iters, step)
        assert _same_bits(on._powersgd._ps_buffer, off._powersgd._ps_buffer)
        assert _same_bits(on._powersgd._qs_buffer, off._powersgd._qs_buffer)
        assert _flags(on) == (0, 0)
    with pytest.raises(ValueError, match="before the first aggregate"):
        on.skip_nonfinite = False
    with pytest.raises(ValueError, match="before the first aggregate"):
        off.skip_nonfinite = True


@pytest.mark.parametrize("rank,iters", RANK_ITERS)
def test_finite_steps_are_untouched(rank, iters):
    _finite_case(rank, iters, torch.float32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
def test_finite_steps_are_untouched_other_dtypes(dtype):
    _finite_case(4, 2, dtype)


# ------------------------------------------------------------------ 2. skip semantics against the oracle
def _skip_case(rank, iters, kind, at, dtype=torch.float32, start=0, steps=4):
    """`steps` steps from the oracle's initial P / Q, the input of step `at` poisoned. Returns the
    tensor-cases (step, tensor) the oracle could not arbitrate (module docstring)."""
    if dtype == torch.float64:
        torch.set_default_dtype(torch.float64)
    tol = TOL[dtype]
    psgd = _make(rank, iters, dtype, start, skip_nonfinite=True)
    codec = psgd._powersgd
    ora = _oracle(rank, iters, start)
    assert ora.mask == psgd.is_compressed_mask
    seed = (ora.codec.p_flat.clone(), ora.codec.q_flat.clone())
    _seed_from_oracle(psgd, ora)
    res = [torch.zeros(s, device=DEV, dtype=dtype) for s in SHAPES]
    skipped, twin, gated = 0, None, []
    for t in range(steps):
        fresh = _inputs(2000 + 100 * rank + 10 * iters + t, dtype)
        gd = [r + x.to(DEV) for r, x in zip(res, fresh)]
        if t == at:
            _poison(gd, kind)
        gc = _oracle_inputs(gd)
        g_twin = [g.clone() for g in gd]
        warm = t < start
        p_before, q_before = codec._ps_buffer.clone(), codec._qs_buffer.clone()
        outs = psgd.aggregate(gd)
        torch.cuda.synchronize()
        ctx = (rank, iters, kind, at, str(dtype), t)
        if t == at:
            skipped += 1
            for o in outs:
                assert _all_zero_bits(o), ctx
            for g in gd:
                assert _all_zero_bits(g), ctx
            if warm:  # no codec ran: P / Q are neither read nor reset
                assert _same_bits(codec._ps_buffer, p_before) and _same_bits(codec._qs_buffer, q_before), ctx
                ora.step += 1
            else:
                assert _same_bits(codec._ps_buffer, psgd.reset_p) and _same_bits(codec._qs_buffer, psgd.reset_q), ctx
                ora = _fresh_oracle_like(psgd, rank, iters, start)
                assert _same_bits(ora.codec.p_flat.to(DEV), psgd.reset_p), ctx
            assert _flags(psgd) == (1, skipped), ctx
            twin = _twin(psgd, seed, rank, iters, dtype, start)
        else:
            scales = [g.clone() for g in gc]
            own = [0.0] * len(SHAPES)
            if dtype != torch.float64:  # (an fp64 plan has no higher precision to be held against)
                gc64 = [g.double() for g in gc]
                want64 = O.policy_step(_oracle64(ora, rank, iters, start), gc64)
            want = O.policy_step(ora, gc)  # (leaves the residual in gc)
            if dtype != torch.float64:
                own = _own_error(want, gc, want64, gc64, scales)
            for i, scale in enumerate(scales):
                eo, er = _rel(outs[i], want[i], scale), _rel(gd[i], gc[i], scale)
                ef = _rel(outs[i].double() + gd[i].double(), scale, scale)
                print(f"guard {ctx} tensor {i}: out {eo:.3e} res {er:.3e} (bound {tol:.0e}; the oracle's own "
                      f"fp32 error {own[i]:.3e}), out + res - in {ef:.3e}")
                if own[i] > 0.1 * tol:  # the reference cannot arbitrate this tensor-case at this bound
                    gated.append((t, i))
                    assert t > at + 1 or (t > 0 and t < at), ctx  # never a step from a fresh state
                    check(ef, TOL_EF[dtype], *ctx, i, "error feedback")
                    continue
                check(eo, tol, *ctx, i, "out")
                check(er, tol, *ctx, i, "res")
            assert _flags(psgd) == (0, skipped), ctx
            assert [psgd.step_counter, codec.step_counter] == [ora.step, ora.codec.step], ctx
            _sync_oracle(ora, psgd)
            if twin is not None:  # bit for bit a fresh, unguarded aggregator's step (every tensor)
                o_twin = twin.aggregate(g_twin)
                torch.cuda.synchronize()
                for a, b in zip(outs + gd + [codec._ps_buffer, codec._qs_buffer],
                                o_twin + g_twin + [twin._powersgd._ps_buffer, twin._powersgd._qs_buffer]):
                    assert _same_bits(a, b), ctx
        res = gd
    assert psgd.step_counter == steps and codec.step_counter == steps - min(start, steps)
    if gated:
        print(f"guard {(rank, iters, kind, at, str(dtype))}: oracle comparison gated at (step, tensor) {gated}")
    return gated


@pytest.mark.parametrize("kind", list(POISONS))
@pytest.mark.parametrize("rank,iters", RANK_ITERS)
def test_skip_at_step_1_against_oracle(rank, iters, kind):
    _skip_case(rank, iters, kind, 1)


@pytest.mark.parametrize("kind", list(POISONS))
@pytest.mark.parametrize("rank,iters", [(r, i) for r, i in RANK_ITERS if i == 1])
def test_skip_at_step_2_against_oracle(rank, iters, kind):
    """I = 1: step 1 is an odd step, step 2 an even one."""
    _skip_case(rank, iters, kind, 2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
def test_skip_against_oracle_other_dtypes(dtype):
    _skip_case(4, 2, "nan-joint", 1, dtype)


# ------------------------------------------------------------------ 3. warm-up
@pytest.mark.parametrize("kind", ["nan-joint", "ninf-1d"])
def test_warm_up_step_is_skipped_without_touching_the_factors(kind):
    _skip_case(2, 2, kind, 1, start=2)


# ------------------------------------------------------------------ 4. scan edges
_SLAB_BITS = {
    # dtype: (integer view, poisons, finite values that must pass)
    torch.float32: (torch.int32, [0x7FC00000, 0x7F800000, -0x00800000],  # NaN, +inf, -inf (0xFF800000)
                    [0x7F7FFFFF, 0x00000001, -0x80000000]),              # largest finite, smallest subnormal, -0.0
    torch.bfloat16: (torch.int16, [0x7FC0, 0x7F80, -0x0080],             # (0xFF80)
                     [0x7F7F, 0x0001, -0x8000]),
    torch.float64: (torch.int64, [0x7FF8000000000000, 0x7FF0000000000000, -0x0010000000000000],
                    [0x7FEFFFFFFFFFFFFF, 0x0000000000000001, -0x8000000000000000]),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_scan_edges_of_the_slab(dtype):
    """The warm-up form of psgd_guard_outputs on a slab whose base is one element past an allocation
    (a scalar head before the vectors): each poison at 0, n / 2 and n - 1 is detected and the slab,
    and only the slab, zeroed; the finite extremes pass and nothing is written."""
    if dtype == torch.float64:
        torch.set_default_dtype(torch.float64)
    psgd = _make(2, 1, dtype, skip_nonfinite=True)
    plan = psgd._powersgd._plan
    itype, poisons, finite = _SLAB_BITS[dtype]
    gen = torch.Generator().manual_seed(21)
    verdicts, want, ok = [], [], torch.ones((), dtype=torch.bool, device=DEV)
    for n in (1, 63, 4097, 70001):
        host = torch.randn(n + 2, generator=gen, dtype=torch.float64).to(dtype)
        for bits, bad in [(b, 1) for b in poisons] + [(b, 0) for b in finite]:
            for at in sorted({0, n // 2, n - 1}):
                buf = host.to(DEV)
                view = buf[1:n + 1]  # one element before and one after stay as sentinels
                assert view.data_ptr() % 16 != 0
                view.view(itype)[at] = bits
                before = buf.clone()
                res = torch.full((2,), 5, dtype=torch.int64, device=DEV)
                plan.guard_outputs(None, 0, view.data_ptr(), n, 0, 0, res.data_ptr(), _stream())
                verdicts.append(res)
                want.append([bad, 5 + bad])
                after, b4 = buf.view(itype), before.view(itype)
                ok &= (after[0] == b4[0]) & (after[n + 1] == b4[n + 1])
                ok &= ~after[1:n + 1].any() if bad else (after == b4).all()
    torch.cuda.synchronize()
    assert torch.stack(verdicts).cpu().tolist() == want
    assert bool(ok)


def test_scan_edges_of_the_factors_and_the_counters():
    """The first and last element of P and of Q poisoned directly; result[0] returns to 0 on the
    next finite call and the count keeps the poisoned calls."""
    psgd = _make(4, 2, skip_nonfinite=True)
    codec, u = psgd._powersgd, psgd._unc
    grads = [x.to(DEV) for x in _inputs(31)]
    outs = psgd.aggregate(grads)
    torch.cuda.synchronize()
    assert _flags(psgd) == (0, 0)

    def guard():
        psgd._guard(psgd._table.comp_addr(), codec._slab.data_ptr(), u.slab.data_ptr(), u.numel)
        torch.cuda.synchronize()
        return _flags(psgd)

    count = 0
    for buf in (codec._ps_buffer, codec._qs_buffer):
        for at in (0, buf.numel() - 1):
            for value in (NAN, INF, -INF):
                assert guard() == (0, count)  # finite: the flag went back to 0
                state = (codec._ps_buffer.clone(), codec._qs_buffer.clone())
                buf[at] = value
                count += 1
                assert guard() == (1, count), (at, value)
                assert _same_bits(codec._ps_buffer, psgd.reset_p) and _same_bits(codec._qs_buffer, psgd.reset_q)
                codec._ps_buffer.copy_(state[0])  # (reset_p / reset_q are the state's own draw here)
                codec._qs_buffer.copy_(state[1])
    assert count == 12 and guard() == (0, 12)
    for t in outs + grads:
        assert _all_zero_bits(t)
    # two poisoned calls count as 2 on a fresh aggregator
    other = _make(4, 2, skip_nonfinite=True)
    for t in range(3):
        g = [x.to(DEV) for x in _inputs(32 + t)]
        if t != 1:
            _poison(g, "ninf-1d")
        other.aggregate(g)
    torch.cuda.synchronize()
    assert _flags(other) == (1, 2)


# ------------------------------------------------------------------ 5. store bounds
def _carved(dtype, fill):
    """The gradient tensors as views of one buffer at odd element offsets with sentinels between."""
    total = 1 + sum(math.prod(s) + 2 for s in SHAPES)
    buf = torch.full((total,), fill, dtype=dtype, device=DEV)
    views, inside, off = [], torch.zeros(total, dtype=torch.bool, device=DEV), 1
    for s in SHAPES:
        n = math.prod(s)
        assert off % 2 == 1
        views.append(buf[off:off + n].view(s))
        inside[off:off + n] = True
        off += n + (2 if n % 2 == 0 else 1)  # one sentinel (two where that keeps the next offset odd)
    return buf, views, inside


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zeroing_stays_inside_misaligned_gradient_views(dtype):
    fill = 1.5
    buf_on, g_on, inside = _carved(dtype, fill)
    buf_off, g_off, _ = _carved(dtype, fill)
    esz = buf_on.element_size()
    assert all(v.data_ptr() % esz == 0 for v in g_on)
    assert any(v.data_ptr() % 16 != 0 for v in g_on) and any(v.data_ptr() % 4 != 0 for v in g_on) == (esz == 2)
    on, off = _make(4, 2, dtype, skip_nonfinite=True), _make(4, 2, dtype)
    for step in range(3):
        for a, b, x in zip(g_on, g_off, _inputs(50 + step, dtype)):
            a.copy_(x)
            b.copy_(x)
        if step == 1:
            _poison(g_on, "nan-joint")
        o_on, o_off = on.aggregate(g_on), off.aggregate(g_off)
        torch.cuda.synchronize()
        if step == 1:
            assert _flags(on) == (1, 1)
            assert all(_all_zero_bits(v) for v in g_on) and all(_all_zero_bits(o) for o in o_on)
            assert bool((buf_on[~inside] == fill).all())  # every sentinel is bit-intact
            assert _all_zero_bits(buf_on[inside])
            off = _make(4, 2, dtype)  # the guarded codec is a fresh one now, except for its counters
            off.step_counter, off._powersgd.step_counter = on.step_counter, on._powersgd.step_counter
        else:
            assert _flags(on) == (0, step // 2)
            assert _same_bits(buf_on, buf_off), step
            for a, b in zip(o_on, o_off):
                assert _same_bits(a, b), step


# ------------------------------------------------------------------ 6. with max_grad_norm
def test_with_max_grad_norm():
    both = _make(4, 2, max_grad_norm=1.0, skip_nonfinite=True)
    clip = _make(4, 2, max_grad_norm=1.0)
    for step in range(3):
        new = _inputs(60 + step)
        g_both, g_clip = [x.to(DEV) for x in new], [x.to(DEV) for x in new]
        if step == 1:
            _poison(g_both, "pinf-96x201")
        o_both, o_clip = both.aggregate(g_both), clip.aggregate(g_clip)
        torch.cuda.synchronize()
        if step == 1:
            assert all(_all_zero_bits(t) for t in o_both + g_both)
            assert math.isnan(float(both.last_clip_coef)) and not math.isfinite(float(both.last_grad_norm))
            assert _flags(both) == (1, 1)
            clip = _make(4, 2, max_grad_norm=1.0)
            clip.step_counter, clip._powersgd.step_counter = both.step_counter, both._powersgd.step_counter
        else:
            assert float(both.last_clip_coef) < 1.0
            for a, b in zip(o_both + g_both + [both.last_grad_norm, both.last_clip_coef],
                            o_clip + g_clip + [clip.last_grad_norm, clip.last_clip_coef]):
                assert _same_bits(a, b), step
            assert _flags(both) == (0, step // 2)


# ------------------------------------------------------------------ 7. fp32 residual of bf16 gradients
def test_fp32_residual_fused_runs_three_stages_and_skips():
    cfg = _config(4, 2)
    params = [torch.zeros(s, device=DEV, dtype=torch.bfloat16) for s in SHAPES]
    assert Fp32ResidualPowerSGD(params, cfg, fused=True).fused_folds()[1] == 1
    agg = Fp32ResidualPowerSGD(params, cfg, fused=True, skip_nonfinite=True)
    assert agg.skip_nonfinite is True and agg.inner.skip_nonfinite is True
    assert agg.fused_folds() == (0, 0)
    twin = None
    for step in range(3):
        new = _inputs(70 + step, torch.bfloat16)
        grads = [x.to(DEV) for x in new]
        if step == 1:
            _poison(grads, "nan-last")
        assert agg.fused_folds() == (0, 0)
        outs = agg.aggregate(grads)
        torch.cuda.synchronize()
        assert all(_all_zero_bits(g) for g in grads)  # consumed
        if step == 1:
            assert _flags(agg) == (1, 1)
            assert _all_zero_bits(agg.residual)
            assert all(o.dtype == torch.bfloat16 and _all_zero_bits(o) for o in outs)
            twin = Fp32ResidualPowerSGD(params, cfg)  # a fresh aggregator whose counters were advanced
            twin.inner.step_counter, twin.inner._powersgd.step_counter = 2, 2
        if step == 2:
            assert _flags(agg) == (0, 1)
            want = twin.aggregate([x.to(DEV) for x in new])
            torch.cuda.synchronize()
            for a, b in zip(outs, want):
                assert _same_bits(a, b)
            assert _same_bits(agg.residual, twin.residual)


# ------------------------------------------------------------------ 8. optimizer_step
def test_optimizer_step_with_sgd_does_not_move_on_a_skipped_step():
    gen = torch.Generator().manual_seed(80)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in SHAPES]
    agg = PowerSGD(params, _config(4, 2), skip_nonfinite=True)
    opt = torch.optim.SGD(params, lr=0.5)
    for step in range(2):
        for p, x in zip(params, _inputs(81 + step)):
            p.grad = x.to(DEV)
        if step == 1:
            _poison([p.grad for p in params], "nan-joint")
        before = [p.detach().clone() for p in params]
        optimizer_step(opt, agg)
        torch.cuda.synchronize()
        moved = [not _same_bits(p.detach(), b) for p, b in zip(params, before)]
        if step == 0:
            assert all(moved) and _flags(agg) == (0, 0)
        else:
            assert not any(moved) and _flags(agg) == (1, 1)
            assert all(_all_zero_bits(p.grad) for p in params)


# ------------------------------------------------------------------ 9. the DDP hook
def _hook_child(_, init):
    from test_gpu_ddp_clip import _Child
    from test_gpu_ddp_direct import _fresh, _mcr

    ch = _Child(init)
    try:
        cfg = Config(4, _mcr(4, 2), 2, 0)
        ddp, state = ch.model(cfg, 3, skip_nonfinite=True)
        assert state.skip_nonfinite is True and state.powersgd.skip_nonfinite is True
        state.direct_store = True  # asked for, never taken while the guard is set
        params = list(ddp.module.parameters())
        for t in range(3):
            assert state.direct_store_applies() is False and state.fused_folds() == (0, 0)
            cs = [g.to(ch.dev) for g in _fresh(t)]
            if t == 1:
                cs[2].view(-1)[5] = NAN
            ddp(cs).backward()
            torch.cuda.synchronize()
            grads = [p.grad.clone() for p in params]
            for p in params:
                p.grad = None
            if t == 1:
                assert (int(state.last_step_skipped), int(state.skipped_steps)) == (1, 1)
                assert all(_all_zero_bits(g) for g in grads)  # what the buckets handed back
                assert _all_zero_bits(state.residual)
                codec = state.powersgd._powersgd
                assert _same_bits(codec._ps_buffer, state.powersgd.reset_p)
                assert _same_bits(codec._qs_buffer, state.powersgd.reset_q)
            else:
                assert (int(state.last_step_skipped), int(state.skipped_steps)) == (0, t // 2)
                assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads if g.numel() > 1)
        state.powersgd.close()
    finally:
        ch.close()


def test_hook_hands_back_zero_buckets_on_a_skipped_step(tmp_path):
    from test_gpu_ddp_direct import _init

    torch.multiprocessing.spawn(_hook_child, args=(_init(tmp_path),), nprocs=1, join=True)


# ------------------------------------------------------------------ 10. world size 3
def _world3_child(_, init):
    from oracle import multiworker as MW
    from test_gpu_ddp_direct import STUB

    os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
    os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
    os.environ["PSGD_STUB_MODE"] = "sum"
    world, rank, iters, at = 3, 4, 2, 1
    torch.cuda.set_device(DEV)
    torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
    try:
        psgd = _make(rank, iters, skip_nonfinite=True)
        codec = psgd._powersgd
        # the library's own communicator, created through the stand-in at world 3: its SUM
        # all-reduce writes 3 x the buffer, the SUM over three ranks holding identical gradients
        codec._comm = _lib.Comm(world, 0, _lib.comm_unique_id(), 0)

        def workers(fresh_from=None):
            states = [_oracle(rank, iters) for _ in range(world)]
            if fresh_from is not None:
                for st in states:
                    st.step, st.codec.step = fresh_from.step_counter, fresh_from._powersgd.step_counter
            return states

        states = workers()
        _seed_from_oracle(psgd, states[0])
        res = [torch.zeros(s, device=DEV) for s in SHAPES]
        for t in range(4):
            fresh = _inputs(3000 + t)
            gd = [r + x.to(DEV) for r, x in zip(res, fresh)]
            if t == at:
                _poison(gd, "nan-joint")
            scale = _oracle_inputs([r + x.to(DEV) for r, x in zip(res, fresh)])
            gc = [_oracle_inputs(gd) for _ in range(world)]
            outs = psgd.aggregate(gd)
            torch.cuda.synchronize()
            if t == at:
                assert all(_all_zero_bits(x) for x in outs + gd)
                assert _same_bits(codec._ps_buffer, psgd.reset_p) and _same_bits(codec._qs_buffer, psgd.reset_q)
                assert _flags(psgd) == (1, 1)
                states = workers(psgd)
            else:
                gc64 = [[g.double() for g in w] for w in gc]
                want64 = MW.run_workers([_oracle64(st, rank, iters) for st in states], gc64)
                want = MW.run_workers(states, gc)
                own = _own_error(want[0], gc[0], want64[0], gc64[0], scale)
                for i in range(len(SHAPES)):
                    eo, er = _rel(outs[i], want[0][i], scale[i]), _rel(gd[i], gc[0][i], scale[i])
                    print(f"guard world 3 step {t} tensor {i}: out {eo:.3e} res {er:.3e} (the oracle's own fp32 "
                          f"error {own[i]:.3e})")
                    if own[i] > 0.1 * TOL[torch.float32]:  # (module docstring; never a step from a fresh state)
                        assert t == at + 2, (t, i)
                        continue
                    check(eo, TOL[torch.float32], "w3", t, i, "out")
                    check(er, TOL[torch.float32], "w3", t, i, "res")
                assert _flags(psgd) == (0, 1 if t > at else 0)
                for st in states:
                    _sync_oracle(st, psgd)
            res = gd
        psgd.close()
    finally:
        torch.distributed.destroy_process_group()


def test_world_size_3_through_the_stand_in_communicator(tmp_path):
    from test_gpu_ddp_direct import _init

    torch.multiprocessing.spawn(_world3_child, args=(_init(tmp_path),), nprocs=1, join=True)
