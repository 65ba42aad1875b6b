"""``Fp32ResidualPowerSGD(..., fused=True)`` in a process group that runs over the library's own
communicator (psgd_aggregate_mixed_comm: the bf16 averages stored by the final pass of the W > 1
sequence, the flat tail staged in fp32 around its collective) against the three-stage flow of the
same build on the same communicator (``fused=False``: run-table ADD, psgd_aggregate_comm on the
fp32 residual, run-table GATHER).

The fused call is defined as that sequence, so there is no tolerance: ``torch.equal`` on raw bits,
after every step, of the bf16 outputs, the fp32 residual and the codec's ``_ps_buffer`` /
``_qs_buffer``; the consumed gradients must be +0.0 everywhere, and two fused runs must agree.

World size W runs on ONE GPU through the stand-in collective library (tests/stubs/rccl_stub.hip,
set up as tests/test_gpu_rccl_stub.py does: a spawned child, a one-rank gloo group over a file
store, the codec's communicator created through the stand-in at world W). Its SUM writes W x the
buffer, the SUM over W ranks holding identical gradients. W = 3 is there because x / 3 and
alpha = float(1 / 3.0) are inexact: a multiply in place of the division, or a swapped term set,
changes bits. One child per world size loops over rank x iterations x gradient placement.

Shapes, min_compression_rate, the gradient recipe (with its -0.0 elements) and the two placements
(separate tensors; 2-byte-aligned views at odd element offsets) are those of
tests/test_gpu_fp32_residual_fused.py: the smallest that reach the vector and element paths of
the apply tiles, a ragged last tile, and at least one uncompressed tensor at every rank."""
import ctypes
import os

import pytest
import torch

from parity_log import check

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3), (40,), (257, 260), (1, 96), (96, 1)]
STEPS = 4
TOL_STEP, TOL_FREE, TOL_BF16 = 1e-5, 1e-4, 4e-3  # the bounds of tests/test_gpu_fp32_residual.py
CASES = [(rank, iters, odd) for rank in (1, 2, 4) for iters in (1, 2, 3) for odd in (False, True)]


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


def _place(fresh, odd: bool, dev):
    """The step's gradients on the device: separate tensors, or views at odd element offsets of
    one flat bf16 buffer (whose base is 4-byte aligned or better: every view is 2-byte aligned only)."""
    if not odd:
        return [g.to(dev) for g in fresh]
    total = sum(g.numel() + 2 for g in fresh) + 1
    flat = torch.zeros(total, dtype=BF16, device=dev)
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


class _Child:
    """The child's side of a case: the stub as the library's collective library, a one-rank gloo
    group (it only makes is_distributed() true), one communicator of world `world`."""

    def __init__(self, init, world, env=None):
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
        os.environ.update(env or {})
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
        self.world = world
        self.stub = ctypes.CDLL(STUB)  # the same handle the library opened: one call counter
        self.stub.psgd_stub_calls.restype = ctypes.c_longlong

    def comm(self):
        from powersgd_amd import _lib

        return _lib.Comm(self.world, 0, _lib.comm_unique_id(), 0)

    def aggregator(self, rank, iters, fused):
        from powersgd_amd import Config, Fp32ResidualPowerSGD

        agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=BF16, device=self.dev) for s in SHAPES],
                                   Config(rank, _mcr(rank, iters), iters, 0), fused=fused)
        agg.inner._powersgd._comm = self.comm()
        mask = agg.is_compressed_mask
        assert any(mask) and not all(mask), mask
        return agg

    def flow(self, rank, iters, odd, fused, steps=STEPS):
        """`steps` steps of one aggregator; per step the raw bits of everything observable and the
        stub's collective count."""
        agg = self.aggregator(rank, iters, fused)
        rec = []
        for t in range(steps):
            grads = _place(_fresh(t), odd, self.dev)
            folds = agg.fused_folds()
            codec = agg.inner._powersgd
            final = codec._plan.fused_final(codec.step_counter, False)  # this step's final pass at W > 1
            n0 = self.stub.psgd_stub_calls()
            out = agg.aggregate(grads)
            torch.cuda.synchronize()
            rec.append({
                "folds": folds,
                "final": final,
                "calls": self.stub.psgd_stub_calls() - n0,
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


def _init(tmp_path):
    return f"file://{tmp_path}/store"


# ------------------------------------------------------------------ cases 1, 2 and 5
def _bitwise(_, init, world):
    ch = _Child(init, world)
    finals = set()
    try:
        for rank, iters, odd in CASES:
            ctx = (world, rank, iters, odd)
            ref = ch.flow(rank, iters, odd, False)  # the reference: computed once, never modified
            assert [r["folds"] for r in ref] == [(0, 0)] * STEPS, ctx  # fused=False never folds
            one = ch.flow(rank, iters, odd, True)
            assert [r["folds"] for r in one] == [(0, 1)] * STEPS, (ctx, [r["folds"] for r in one])
            _same(one, ref, ctx)
            two = ch.flow(rank, iters, odd, True)
            _same(two, one, (ctx, "second fused run"))
            assert any(bool(r["residual"].any()) for r in one), ctx  # the residuals are non-trivial
            # one collective per power iteration plus the flat tail grouped with the last one
            # (every case has an uncompressed tensor): the three-stage flow's count
            assert [r["calls"] for r in one] == [iters + 1] * STEPS, (ctx, [r["calls"] for r in one])
            assert [r["calls"] for r in ref] == [iters + 1] * STEPS, (ctx, [r["calls"] for r in ref])
            finals |= {(rank, r["final"]) for r in one}
        # both final passes of the communicator sequence were reached: the two-term-set apply pass
        # (every rank bucket) and the output pass after a fused k_final_odd (rank buckets 1 and 2)
        assert {(1, 0), (2, 0), (4, 0), (1, 1), (2, 1)} <= finals, finals
    finally:
        ch.close()


@pytest.mark.parametrize("world", [3, 4])
def test_fused_equals_three_stage_flow_bitwise_world_w(world, tmp_path):
    """Case 1: bit for bit at W = 3 and W = 4, every rank bucket, 1-3 iterations, both placements."""
    torch.multiprocessing.spawn(_bitwise, args=(_init(tmp_path), world), nprocs=1, join=True)


def test_fused_equals_three_stage_flow_bitwise_one_rank_communicator(tmp_path):
    """Case 5: a communicator of world 1: the world-size-1 instance and the / 1 flat path inside
    the communicator call."""
    torch.multiprocessing.spawn(_bitwise, args=(_init(tmp_path), 1), nprocs=1, join=True)


def _count(_, init, world):
    ch = _Child(init, world)
    try:
        for iters in (1, 2, 3):
            fused = ch.flow(2, iters, False, True, steps=2)
            plain = ch.flow(2, iters, False, False, steps=2)
            assert [r["folds"] for r in fused] == [(0, 1)] * 2
            assert [r["calls"] for r in fused] == [iters + 1] * 2 == [r["calls"] for r in plain], (iters, fused, plain)
    finally:
        ch.close()


def test_collective_count(tmp_path):
    """Case 2: a fused step makes num_iters_per_step + 1 collective calls (the flat tail grouped
    with the last factor's), the three-stage flow's count."""
    torch.multiprocessing.spawn(_count, args=(_init(tmp_path), 4), nprocs=1, join=True)


# ------------------------------------------------------------------ cases 3 and 4
def _rel(a, b, scale) -> float:
    return float((a.detach().double().cpu() - b.double()).norm()) / max(float(scale.double().norm()), 1e-30)


def _vs_oracle(ch, rank, iters, steps, log):
    """The fused flow against W free-running reference workers on the upcast inputs (the stub sums
    W identical ranks, so every oracle worker gets the same inputs). Returns the largest error."""
    from oracle import multiworker as MW
    from oracle import powersgd_oracle as O

    world = ch.world
    agg = ch.aggregator(rank, iters, True)
    codec = agg.inner._powersgd
    oracles = []
    for _ in range(world):
        st = O.policy_init([torch.zeros(s) for s in SHAPES], rank, _mcr(rank, iters), iters, 0)
        st.codec.p_flat.copy_(codec._ps_buffer.cpu())
        st.codec.q_flat.copy_(codec._qs_buffer.cpu())
        oracles.append(st)
    ora_res = [[torch.zeros(s) for s in SHAPES] for _ in range(world)]
    worst = 0.0
    for t in range(steps):
        fresh = _fresh(t)
        grads = _place(fresh, False, ch.dev)
        assert agg.fused_folds() == (0, 1)
        out = agg.aggregate(grads)
        torch.cuda.synchronize()
        gc = [[r + g.float() for r, g in zip(ora_res[w], fresh)] for w in range(world)]
        ins = [x.clone() for x in gc[0]]
        want = MW.run_workers(oracles, gc)
        tol = TOL_STEP if t == 0 else TOL_FREE
        for i in range(len(SHAPES)):
            er = _rel(agg.views[i], gc[0][i], ins[i])
            eo = _rel(out[i].float(), want[0][i], ins[i])
            worst = max(worst, er, eo)
            if log:
                check(er, tol, "mixed_comm", rank, iters, world, t, i, "fp32res-residual")
                check(eo, TOL_BF16, "mixed_comm", rank, iters, world, t, i, "fp32res-avg")
        ora_res = gc
    agg.close()
    return worst


def _oracle(_, init):
    ch = _Child(init, 4)
    try:
        _vs_oracle(ch, 2, 2, 3, True)
    finally:
        ch.close()


def test_against_w_reference_workers(tmp_path):
    """Case 3: rank 2, two iterations, W = 4, three steps against W reference workers."""
    torch.multiprocessing.spawn(_oracle, args=(_init(tmp_path),), nprocs=1, join=True)


def _skip_flat(_, init, q):
    # the flat tail is the last collective of step 0: index num_iters_per_step = 2
    ch = _Child(init, 4, {"PSGD_STUB_MODE": "skip", "PSGD_STUB_SKIP_AT": "2"})
    try:
        q.put(_vs_oracle(ch, 1, 2, 1, False))
    finally:
        ch.close()


def test_negative_control_lost_flat_collective(tmp_path):
    """Case 4: a collective library that drops the flat tail's all-reduce must show against the
    reference workers: the fused flat path really goes through the collective."""
    ctx = torch.multiprocessing.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_skip_flat, args=(0, _init(tmp_path), q))
    p.start()
    err = q.get(timeout=300)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert err > 1e-2, err


# ------------------------------------------------------------------ case 6
def _refusals(_, init):
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    ch = _Child(init, 4)
    try:
        dev = ch.dev
        shapes = [(300, 520), (130, 67)]
        stream = torch.cuda.current_stream(dev).cuda_stream

        def state(codec, dt):
            gen = torch.Generator().manual_seed(5)
            grads = [torch.randn(s, generator=gen).to(BF16).to(dev) for s in shapes]
            resid = [torch.randn(s, generator=gen).to(dev) for s in shapes]
            out = torch.full((sum(torch.Size(s).numel() for s in shapes),), 3.0, dtype=BF16, device=dev)
            return grads, resid, out, grads + resid + [out, codec._ps_buffer, codec._qs_buffer]

        def unchanged(live, keep, n0, ctx):
            torch.cuda.synchronize()
            for a, b in zip(live, keep):
                assert torch.equal(_bits(a) if a.dtype == BF16 else a, _bits(b) if b.dtype == BF16 else b), ctx
            assert ch.stub.psgd_stub_calls() == n0, ctx

        for what in ("rank8", "bf16", "wide"):
            rank = {"rank8": 8, "bf16": 2, "wide": 64}[what]
            dt = BF16 if what == "bf16" else torch.float32
            codec = BasicPowerSGD([torch.zeros(s, dtype=dt, device=dev) for s in shapes], BasicConfig(rank, 2))
            assert codec._plan.is_wide() == (what == "wide")
            for w in (1, 4):
                assert codec._plan.mixed_folds_comm(0, w) == (0, 0) and codec._plan.mixed_folds_comm(1, w) == (0, 0)
            comm = ch.comm()
            grads, resid, out, live = state(codec, dt)
            keep = [x.clone() for x in live]
            gp = _lib.ptr_array([g.data_ptr() for g in grads])
            rp = _lib.ptr_array([r.data_ptr() for r in resid])
            n0 = ch.stub.psgd_stub_calls()
            with pytest.raises(ValueError, match="psgd_aggregate_mixed"):
                codec._plan.aggregate_mixed_comm(ctypes.addressof(gp), ctypes.addressof(rp), out.data_ptr(), 0, comm,
                                                 stream)
            unchanged(live, keep, n0, what)

        # a poisoned communicator (a psgd_aggregate_comm call that failed past its argument checks:
        # a null gradient pointer, refused before anything runs) is refused at entry
        codec = BasicPowerSGD([torch.zeros(s, device=dev) for s in shapes], BasicConfig(2, 2))
        assert codec._plan.mixed_folds_comm(0, 4) == (0, 1)
        comm = ch.comm()
        grads, resid, out, live = state(codec, torch.float32)
        f32_out = torch.zeros(out.numel(), device=dev)
        bad = _lib.ptr_array([0] * len(shapes))
        with pytest.raises(ValueError, match="null gradient pointer"):
            codec._plan.aggregate_comm(ctypes.addressof(bad), f32_out.data_ptr(), 0, None, None, 0, comm, stream)
        keep = [x.clone() for x in live]
        gp = _lib.ptr_array([g.data_ptr() for g in grads])
        rp = _lib.ptr_array([r.data_ptr() for r in resid])
        n0 = ch.stub.psgd_stub_calls()
        with pytest.raises(RuntimeError, match="communicator unusable"):
            codec._plan.aggregate_mixed_comm(ctypes.addressof(gp), ctypes.addressof(rp), out.data_ptr(), 0, comm, stream)
        unchanged(live, keep, n0, "poisoned")
    finally:
        ch.close()


def test_direct_call_refusals_touch_nothing(tmp_path):
    """Case 6: rank bucket 8, a bf16 plan and a wide plan are refused with PSGD_ERR_VALUE, a
    poisoned communicator at entry; gradients, residual, outputs, P/Q and the collective count
    stay as they were."""
    torch.multiprocessing.spawn(_refusals, args=(_init(tmp_path),), nprocs=1, join=True)
