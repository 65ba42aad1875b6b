"""Matrices whose own rank r = min(n, m, rank) lies below the plan's rank bucket, in every bucket
(8, 16, 32, wide), against the CPU oracle through the public entries: ``PowerSGD.aggregate`` on
fp32, bf16 and fp64 gradients and ``Fp32ResidualPowerSGD`` (three-stage and fused). World size 2
is in tests/test_gpu_capped_rank_multi.py, which takes the shape set, the inputs and the skip table
from here.

One anchor matrix makes the bucket the requested one; every other matrix is capped by its rows or
columns. With min_compression_rate = 0.01 every tensor is compressed (asserted against the
oracle's mask), the 1-D tensor as a [41, 1] matrix of rank 1, so the tensors behind it sit at an
output offset that is no multiple of 4. The gradient of tensor 2 is a view one element into its
allocation: psgd_step.cpp's alignment test then takes it off the vector layout (``vec_now`` differs
from ``base_vec``) while tensor 1, the other matrix of its group, stays on it.

Layout the plan gives each matrix (psgd_plan_create ``base_vec``; V = 4-column vector layout, s =
scalar layout) and the term of ``base_vec`` / of geometry()'s ``d.vec || (rbucket >= 16 && m % 4
== 0)`` that decides it:

    #   shape         [n, m]      own r        out_off % 4   bucket 8   16 / 32             wide
    0   (160, 136)    [160, 136]  rank         0             V          s: r > 8, row quads  s: r > 8
    1   (3, 200)      [3, 200]    3            0             V          s: bucket, quads     V
    2   (3, 200)      [3, 200]    3            0 (grad + 1)  V -> s     s: bucket, quads     V
    3   (8, 64)       [8, 64]     8            0             V          s: bucket, quads     V
    4   (64, 8)       [64, 8]     8            0             V          s: bucket, quads     V
    5   (12, 100)     [12, 100]   min(12,rank) 0             V (r = 8)  s: r > 8, quads      s: r > 8
    6   (1, 96)       [1, 96]     1            0             V          s: bucket, quads     V
    7   (96, 1)       [96, 1]     1            0             s: m % 4   s: m % 4             s: m % 4
    8   (6, 4, 3, 3)  [6, 36]     6            0             V          s: bucket, quads     V
    9   (41,)         [41, 1]     1            0             s: m % 4   s: m % 4             s: m % 4
    10  (8, 64)       [8, 64]     8            1             s: offset  s: offset, quads     s: offset
    11  (5, 201)      [5, 201]    5            1             s: m % 4   s: m % 4             s: m % 4
    12  (200, 3)      [200, 3]    3            2             s: m % 4   s: m % 4             s: m % 4
    13  (100, 13)     [100, 13]   min(13,rank) 2             s: m % 4   s: m % 4             s: m % 4

("quads": the even product streams 16-byte row quads on the matrix cores although the layout is
scalar; fp64 plans are scalar throughout.) Groups: [3, 200] and [8, 64] hold two matrices each.

Every step is compared from an identical state: P / Q are drawn on the CPU, copied into the GPU
object, the oracle is initialised from the GPU object's buffers and re-synchronised from them after
every step (degenerate panels make the free-running state ill-posed). Two steps per case; with one
iteration per step that is an even step followed by an odd one.

Tolerances are the project's: ||ours - oracle||_F <= TOL * ||input||_F per tensor with TOL_STEP =
1e-5 (fp32), TOL_BF16 = 4e-3 (bf16 gradients or bf16 averages; the oracle runs on the bf16-rounded
inputs) and TOL_F64 = 1e-12 (tests/test_gpu_f64.py's constant: a length-200 dot product rounds at
200 * 2^-53 = 2.2e-14 relative, the bound is some forty times that). Error feedback: ||out +
residual - input||_F <= 1e-6 * ||input||_F (1e-12 in fp64); where the output or the residual is
stored in bf16 the bound is that rounding, 2^-9 (||out|| + ||residual||) <= 2^-8.5 ||input|| =
2.8e-3, checked against TOL_BF16.

Write coverage: before every step the output slab the step is about to fill (the codec's, the bf16
slab of the fp32-residual aggregator, the fused step's) is filled with NaN through the slab's own
``get`` (a buffer nobody holds is handed out again, asserted by pointer); afterwards all of it
must be finite.

Well-posedness. Where iters * r > min(n, m) the later iterations work on a residual that is pure
rounding. ``PYTHONPATH=. python tests/test_gpu_capped_rank.py`` runs, on the CPU alone, the oracle
in fp32 and in float64 on every case's inputs from the same state (step 1 from the fp32 oracle's
state after step 0) and lists the tensor-cases (kind, rank, iters, step, tensor) where the two differ
by more than a tenth of the tolerance; SKIP below is its literal output, and such a tensor-case
keeps the mask assertion, the write coverage and the error-feedback identity. An fp64 plan has no
higher precision to be held against, so it leaves out what the fp32 run of the same case leaves
out. The share is 6 of 1400 tensor-cases here (0.4 %) and 0 of 168 in the world-size-2 file: the
[12, 100] matrix at rank 8 with two or three iterations, at step 1 (4e-2 between fp32 and float64 at
I = 2, 8e-6 at I = 3). Within one step a rounding-decided panel contributes about 1e-7 * ||input||
in absolute terms, which is why nothing else is listed: the oracle's own fp32 noise on the
tensor-cases that are compared is at most 0.06 of their bound (6e-7).

Observed on an MI355X (profiles/capped_rank/figures.txt): fp32 at most 6.2e-7
(bound 1e-5), bf16 gradients 1.9e-3 and the bf16 averages of the fp32-residual flows 1.8e-3 (4e-3),
their fp32 residual 6.5e-7 (1e-5), fp64 1.0e-15 (1e-12), error feedback 4.5e-8 (1e-6). With the
``bucket_vec`` term of ``base_vec`` taken out again (a scratch build, profiles/capped_rank/
bucket_vec_reverted.txt) the rank 12 - 32 cases fail in the oracle comparison and in the write
coverage."""
import contextlib

import pytest
import torch

from oracle import powersgd_oracle as O
from parity_log import record
from powersgd_amd import Config, Fp32ResidualPowerSGD, PowerSGD
from powersgd_amd.workloads import hash_tensors

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL_STEP, TOL_BF16, TOL_F64 = 1e-5, 4e-3, 1e-12
TOL_EF = 1e-6
MCR = 0.01
BF16 = torch.bfloat16

SHAPES = [(160, 136), (3, 200), (3, 200), (8, 64), (64, 8), (12, 100), (1, 96), (96, 1), (6, 4, 3, 3), (41,),
          (8, 64), (5, 201), (200, 3), (100, 13)]
OFFSET_GRAD = 2  # this tensor's gradient starts one element into its allocation
STEPS = 2
# (rank, iters): buckets 8, 16 (ranks 12 and 16), 32 (24 and 32), 64 (40 and 64), 128; I = 1 (an even
# step, then an odd one), 2 (even + odd) and 3 (more than one output term); iters * rank <= 136
CASES = [(8, 1), (8, 2), (8, 3), (12, 2), (16, 1), (16, 2), (16, 3), (24, 3), (32, 1), (32, 2), (32, 3), (40, 3), (64, 1),
         (64, 2), (128, 1)]
CASES_F64 = [(8, 1), (8, 3), (16, 1), (16, 2), (16, 3)]
# kind -> {(rank, iters, step, tensor)} left out of the oracle comparison: the output of
# `PYTHONPATH=. python tests/test_gpu_capped_rank.py` (CPU, oracle alone). All of them are tensor 5,
# [12, 100], at rank 8 (own rank 8) with iters * r = 16 or 24 > n = 12, at step 1: the P panel
# step 0 leaves has four columns of rounding noise, and its QR differs by 4e-2 between fp32 and float64
SKIP = {"f32": {(8, 2, 1, 5), (8, 3, 1, 5)}, "bf16": {(8, 2, 1, 5)}, "res32": {(8, 2, 1, 5), (8, 3, 1, 5)},
        "f64": {(8, 3, 1, 5)}, "w2stub": set(), "w2ipc": set()}


def bucket_of(rank):
    own = max(min(rank, s[0], int(torch.Size(s[1:]).numel())) for s in SHAPES if len(s) > 1)
    return 1 << (own - 1).bit_length()


def matrix_dims(shape):
    return shape[0], int(torch.Size(shape[1:]).numel())


def inputs(rank, iters, step, worker=0):
    """The fp32 gradients of one step (CPU), one hash stream per tensor."""
    seed = 5000 + ((rank * 8 + iters) * 4 + step) * 4 + worker
    return [torch.from_numpy(f) for f in hash_tensors(SHAPES, seed=seed)]


@contextlib.contextmanager
def default_dtype(dtype):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(prev)


def oracle_state(rank, iters, dtype=torch.float32):
    """The oracle's policy state with P / Q drawn on the CPU (fp32 values, also for float64)."""
    with default_dtype(torch.float32):
        st = O.policy_init([torch.zeros(s) for s in SHAPES], rank, MCR, iters, 0)
    if dtype != torch.float32:
        with default_dtype(dtype):
            wide = O.policy_init([torch.zeros(s) for s in SHAPES], rank, MCR, iters, 0)
        wide.codec.p_flat.copy_(st.codec.p_flat)
        wide.codec.q_flat.copy_(st.codec.q_flat)
        st = wide
    assert all(st.mask)
    return st


def rel(a, b, scale) -> float:
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(float(scale.double().norm()), 1e-300)


def load_state(codec, ora):
    """The oracle's P / Q into the GPU object, then the oracle from the GPU object's buffers."""
    codec._ps_buffer.copy_(ora.codec.p_flat.to(codec._ps_buffer.dtype))
    codec._qs_buffer.copy_(ora.codec.q_flat.to(codec._qs_buffer.dtype))
    sync_state(ora, codec)


def sync_state(ora, codec):
    ora.codec.p_flat.copy_(codec._ps_buffer.cpu())
    ora.codec.q_flat.copy_(codec._qs_buffer.cpu())


def to_device(tensors, dtype):
    """Device gradients; tensor OFFSET_GRAD as a view one element into an aligned allocation."""
    out = []
    for i, x in enumerate(tensors):
        x = x.to(dtype)
        if i == OFFSET_GRAD:
            buf = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
            g = buf[1:].view(x.shape)
            g.copy_(x)
            assert buf.data_ptr() % 16 == 0 and g.data_ptr() % 16 == x.element_size() and g.is_contiguous()
            out.append(g)
        else:
            out.append(x.to(DEV))
    return out


def poison(slab):
    """Fill the buffer the slab will hand out next with NaN; its address."""
    views = slab.get()
    slab.flat.fill_(float("nan"))
    ptr = slab.data_ptr()
    del views
    return ptr


def all_finite(slab) -> bool:
    return bool(torch.isfinite(slab.flat).all())


class Findings(list):
    """The failed checks of one step, raised together at its end: a defect then shows which tensors
    it reaches and through which checks (write coverage, identity, oracle), not the first alone."""

    def check(self, err, tol, *ctx):
        record(err, tol, *ctx)
        if not err <= tol:  # NaN fails
            self.append((ctx, float(err), tol))

    def expect(self, ok, *ctx):
        if not ok:
            self.append(ctx)

    def done(self):
        assert not self, f"{len(self)} failed checks: " + "; ".join(str(f) for f in self[:16])


def check_plan(codec, rank):
    """The plan has the bucket asked for and the groups (own ranks, counts) of the docstring's table."""
    bucket = bucket_of(rank)
    assert codec._plan.is_wide() == (bucket > 32)
    want = {}
    for s in SHAPES:
        n, m = matrix_dims(s)
        want[(n, m)] = want.get((n, m), 0) + 1
    got = [tuple(int(v) for v in g) for g in codec._plan.groups()]
    assert got == [(n, m, min(rank, n, m), c) for (n, m), c in want.items()], got
    assert got[0][2] == rank  # the anchor alone reaches the requested rank ...
    if bucket >= 16:  # ... and every other matrix is capped below the bucket
        assert all(g[2] < bucket for g in got[1:])
    return bucket


def _plain(kind, rank, iters, dtype, tol, tol_ef):
    """PowerSGD.aggregate on `dtype` gradients, two steps, each from the oracle's state."""
    odt = torch.float64 if dtype == torch.float64 else torch.float32
    psgd = PowerSGD([torch.zeros(s, device=DEV, dtype=dtype) for s in SHAPES], Config(rank, MCR, iters, 0))
    codec = psgd._powersgd
    ora = oracle_state(rank, iters, odt)
    assert psgd.is_compressed_mask == ora.mask
    check_plan(codec, rank)
    load_state(codec, ora)
    for t in range(STEPS):
        x = [v.to(dtype) for v in inputs(rank, iters, t)]  # what the GPU sees, rounded
        gd = to_device(x, dtype)
        gc = [v.to(odt).clone() for v in x]
        ptr = poison(codec._slab)
        od = psgd.aggregate(gd)
        torch.cuda.synchronize()
        assert od[0].data_ptr() == ptr, "the step wrote another buffer than the one filled with NaN"
        found = Findings()
        found.expect(all_finite(codec._slab), kind, rank, iters, t, "output slab not fully written")
        out = [o.cpu() for o in od]
        del od
        oc = O.policy_step(ora, gc)
        for i, v in enumerate(x):
            ctx = (kind, rank, iters, t, i, SHAPES[i])
            assert out[i].dtype == dtype, ctx
            found.expect(bool(torch.isfinite(out[i]).all()), *ctx, "output not fully written")
            found.expect(bool(torch.isfinite(gd[i]).all()), *ctx, "residual not finite")
            ef = rel(out[i].double() + gd[i].double().cpu(), v, v)
            eo, er = rel(out[i], oc[i], v), rel(gd[i], gc[i], v)
            print(f"{kind} rank {rank} iters {iters} step {t} tensor {i}: out {eo:.3e} res {er:.3e} ef {ef:.3e}")
            found.check(ef, tol_ef, *ctx, "ef-identity")
            if (rank, iters, t, i) not in SKIP[kind]:
                found.check(eo, tol, *ctx, "out")
                found.check(er, tol, *ctx, "res")
        found.done()
        sync_state(ora, codec)
    assert bool(torch.isfinite(codec._ps_buffer).all()) and bool(torch.isfinite(codec._qs_buffer).all())


@pytest.mark.parametrize("rank,iters", CASES)
def test_fp32_vs_oracle(rank, iters):
    _plain("f32", rank, iters, torch.float32, TOL_STEP, TOL_EF)


@pytest.mark.parametrize("rank,iters", CASES)
def test_bf16_vs_oracle(rank, iters):
    _plain("bf16", rank, iters, BF16, TOL_BF16, TOL_BF16)


@pytest.mark.parametrize("rank,iters", CASES_F64)
def test_fp64_vs_oracle(rank, iters):
    torch.set_default_dtype(torch.float64)  # P / Q follow it (restored by conftest's fixture)
    _plain("f64", rank, iters, torch.float64, TOL_F64, TOL_F64)


def _residual_flow(rank, iters, fused):
    """Fp32ResidualPowerSGD on bf16 gradients, two steps; per step (bf16 outputs, fp32 residual)."""
    agg = Fp32ResidualPowerSGD([torch.zeros(s, device=DEV, dtype=BF16) for s in SHAPES], Config(rank, MCR, iters, 0),
                               fused=fused)
    codec = agg.inner._powersgd
    ora = oracle_state(rank, iters)
    assert agg.is_compressed_mask == ora.mask
    check_plan(codec, rank)
    if fused:
        # the fused step builds its output slab on first use: one step to have it, then back to step 0
        assert agg.fused_folds()[1] == 1, "the fused entry does not serve this plan"
        agg.aggregate(to_device([v.to(BF16) for v in inputs(rank, iters, STEPS)], BF16))
        torch.cuda.synchronize()
        agg.residual.zero_()
        agg.inner.step_counter = codec.step_counter = 0
    load_state(codec, ora)
    snaps = []
    for t in range(STEPS):
        x = [v.to(BF16) for v in inputs(rank, iters, t)]
        gd = to_device(x, BF16)
        gc = [r.cpu() + v.float() for r, v in zip(agg.views, x)]  # previous residual + fresh: one fp32 add
        scale = [g.clone() for g in gc]
        if fused:
            assert agg.fused_folds()[1] == 1
            slabs = [agg._fused_state["comp_slab"]]
        else:
            assert agg.fused_folds() == (0, 0)
            slabs = [agg._slab, codec._slab]
        ptrs = [poison(s) for s in slabs]
        od = agg.aggregate(gd)
        torch.cuda.synchronize()
        assert od[0].data_ptr() == ptrs[0], "the step wrote another buffer than the one filled with NaN"
        assert [s.data_ptr() for s in slabs] == ptrs
        found = Findings()
        for s in slabs:
            found.expect(all_finite(s), "res32", rank, iters, fused, t, "output slab not fully written")
        out = [o.cpu() for o in od]
        del od
        res = [v.cpu().clone() for v in agg.views]
        oc = O.policy_step(ora, gc)
        for i, g in enumerate(scale):
            ctx = ("res32", rank, iters, fused, t, i, SHAPES[i])
            assert out[i].dtype == BF16 and res[i].dtype == torch.float32, ctx
            found.expect(bool(torch.isfinite(out[i].float()).all()), *ctx, "output not fully written")
            found.expect(bool(torch.isfinite(res[i]).all()), *ctx, "residual not finite")
            found.expect(not bool(gd[i].view(torch.int16).any()), *ctx, "gradients are consumed")
            ef = rel(out[i].double() + res[i].double(), g, g)
            eo, er = rel(out[i], oc[i], g), rel(res[i], gc[i], g)
            print(f"res32 rank {rank} iters {iters} fused {fused} step {t} tensor {i}: out {eo:.3e} res {er:.3e} "
                  f"ef {ef:.3e}")
            found.check(ef, TOL_BF16, *ctx, "ef-identity")
            if (rank, iters, t, i) not in SKIP["res32"]:
                found.check(eo, TOL_BF16, *ctx, "out")
                found.check(er, TOL_STEP, *ctx, "res")
        found.done()
        sync_state(ora, codec)
        snaps.append((out, res, codec._ps_buffer.cpu().clone(), codec._qs_buffer.cpu().clone()))
    return snaps


@pytest.mark.parametrize("rank,iters", CASES)
def test_fp32_residual_vs_oracle(rank, iters):
    """The three-stage flow at every bucket; at buckets 16 and 32 the fused entry as well, against
    the oracle and bit for bit against the three stages."""
    three = _residual_flow(rank, iters, False)
    if bucket_of(rank) not in (16, 32):
        return
    fused = _residual_flow(rank, iters, True)
    for t, (a, b) in enumerate(zip(three, fused)):
        for i in range(len(SHAPES)):
            assert torch.equal(a[0][i].view(torch.int16), b[0][i].view(torch.int16)), (rank, iters, t, i, "output")
            assert torch.equal(a[1][i], b[1][i]), (rank, iters, t, i, "residual")
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), (rank, iters, t, "P/Q")


# ------------------------------------------------------- the skip table, on the CPU alone --
def _flag(kind, rank, iters, t, lo, hi, scale, tols, table, worst):
    """Tensor-cases where the fp32 and the float64 oracle differ by more than a tenth of the bound."""
    for i, g in enumerate(scale):
        for a, b, tol in zip(lo[i], hi[i], tols):
            e = rel(a, b, g)
            if e > tol / 10:
                table[kind].add((rank, iters, t, i))
                print(f"{kind} rank {rank} iters {iters} step {t} tensor {i} {SHAPES[i]}: {e:.3e} > {tol / 10:.0e}")
            else:  # the oracle's own noise floor on the tensor-cases that are compared
                worst[kind] = max(worst.get(kind, 0.0), e / tol)


def _pair_step(s32, gc, world=1):
    """One oracle step in fp32 (advancing `s32`) and one in float64 from the same state and inputs;
    per worker and tensor (output, residual) of each."""
    from oracle import multiworker as MW

    s64 = []
    for st in s32:
        w = oracle_state(st.rank, st.iters, torch.float64)
        w.codec.p_flat.copy_(st.codec.p_flat)
        w.codec.q_flat.copy_(st.codec.q_flat)
        w.codec.step = st.codec.step
        w.step = st.step
        s64.append(w)
    g32 = [[v.clone() for v in g] for g in gc]
    g64 = [[v.double() for v in g] for g in gc]
    o32 = MW.run_workers(s32, g32)
    with default_dtype(torch.float64):
        o64 = MW.run_workers(s64, g64)
    return ([[(o32[w][i], g32[w][i]) for i in range(len(SHAPES))] for w in range(world)],
            [[(o64[w][i], g64[w][i]) for i in range(len(SHAPES))] for w in range(world)])


def derive_skip():
    table = {k: set() for k in SKIP}
    worst, count = {}, {k: 0 for k in SKIP}
    for rank, iters in CASES:
        for kind in ("f32", "bf16", "res32"):
            st = [oracle_state(rank, iters)]
            res = [torch.zeros(s) for s in SHAPES]
            for t in range(STEPS):
                x = inputs(rank, iters, t)
                if kind != "f32":
                    x = [v.to(BF16).float() for v in x]
                if kind == "res32":
                    x = [r + v for r, v in zip(res, x)]
                lo, hi = _pair_step(st, [x])
                tols = {"f32": (TOL_STEP, TOL_STEP), "bf16": (TOL_BF16, TOL_BF16), "res32": (TOL_BF16, TOL_STEP)}[kind]
                _flag(kind, rank, iters, t, lo[0], hi[0], x, tols, table, worst)
                res = [p[1] for p in lo[0]]
                count[kind] += len(SHAPES)
    # fp64 plans: no higher precision to hold the float64 oracle against; a tensor-case whose fp32
    # run is decided by rounding is taken as decided by rounding in float64 too
    table["f64"] = {c for c in table["f32"] if (c[0], c[1]) in CASES_F64}
    count["f64"] = len(CASES_F64) * STEPS * len(SHAPES)
    for kind in ("w2stub", "w2ipc"):
        for rank in (16, 32, 64):
            st = [oracle_state(rank, 2), oracle_state(rank, 2)]
            for t in range(STEPS):
                gc = [inputs(rank, 2, t, w if kind == "w2ipc" else 0) for w in range(2)]
                lo, hi = _pair_step(st, gc, 2)
                for w in range(2):
                    scale = [max(gc[0][i], gc[1][i], key=lambda v: float(v.norm())) for i in range(len(SHAPES))]
                    _flag(kind, rank, 2, t, lo[w], hi[w], scale, (TOL_STEP, TOL_STEP), table, worst)
                count[kind] += len(SHAPES)
    return table, worst, count


if __name__ == "__main__":
    table, worst, count = derive_skip()
    for kind in SKIP:
        print(f"{kind}: {len(table[kind])} of {count[kind]} tensor-cases; the others' worst fp32 - float64 difference is "
              f"{worst.get(kind, 0.0):.3f} of the bound")
    print("SKIP =", {k: sorted(v) for k, v in table.items()})
    total, flagged = sum(count.values()), sum(len(v) for v in table.values())
    print(f"share {flagged} / {total} = {flagged / total:.3f}")
