"""The fused fp32-residual step over the IPC exchange (``PSGD_COMM=ipc``): psgd_aggregate_mixed_ipc
behind ``Fp32ResidualPowerSGD(..., fused=True)`` and psgd_aggregate_mixed_ipc_dst (the DDP hook's
form, called directly here) against the sequences they are defined as on the same build: the
run-table ADD, psgd_aggregate_ipc on the fp32 residual, the run-table GATHER (``fused=False``).

Defined as those sequences, so there is no tolerance: ``torch.equal`` on raw bits, after every
step, of the bf16 outputs, the fp32 residual and the codec's ``_ps_buffer`` / ``_qs_buffer``; the
consumed gradients must be +0.0 everywhere, and two fused runs must agree.

World size W is W real processes on cuda:0 (``torch.multiprocessing.spawn``, a gloo group over a
file store, as tests/test_gpu_ipc.py), and every rank holds its OWN gradients (the seed includes the
rank): the local and the averaged factors differ, which the stand-in collective of
tests/test_gpu_mixed_comm.py (identical ranks) cannot show. W = 3 is there because x / 3 and
alpha = float(1 / 3.0) are inexact.

Shapes, min_compression_rate (at rank 1 raised from 1.99 / I to 2.001 / I, see ``_mcr``: 1-D tensors
stay uncompressed at every rank), the gradient recipe (with its -0.0 elements), the placements and
the raw-bit comparison are those of tests/test_gpu_mixed_comm.py / test_gpu_mixed_comm_dst.py, plus
``(2049,)`` in front of ``(40,)``: an uncompressed tensor of more than kFlatItem = 2048 elements with
a ragged tail (two flat items, the second of one element), which also puts its flat neighbour at an
odd flat offset. One spawn per test, the cases looped inside the workers."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3), (2049,), (40,), (257, 260), (1, 96), (96, 1)]
NUMEL = [torch.Size(s).numel() for s in SHAPES]
STEPS = 3
FLAT_ITEM = 2048  # kFlatItem (psgd_internal.h)
CANARY = 0x7A5B  # a bf16 bit pattern no average of these gradients rounds to in every element
# rank x iterations, the gradient placement alternating
CASES = [(rank, iters, (rank + iters) % 2 == 1) for rank in (1, 2, 4) for iters in (1, 2, 3)]


def _mcr(rank: int, iters: int) -> float:
    # numel / (0.5 I r sum(shape)): a 1-D tensor is exactly 2 / (I r), (1, 96) and (96, 1) are
    # 1.979 / I. The recipe's 1.99 / I at rank 1 compresses every 1-D tensor (2 / I is above it) and
    # leaves only tensors below 199 elements uncompressed, so no flat entry could span two flat
    # items there; 2.001 / I keeps the recipe's compressed set (every other shape is at 47 / I or
    # more) and leaves the 1-D tensors uncompressed at rank 1 as they are at ranks 2 and 4
    return (2.001 if rank == 1 else 1.5) / iters


def _fresh(t: int, rank_id: int):
    """Seeded bf16 gradients of step t on rank `rank_id` (every rank its own) whose scale grows each
    step (non-trivial residuals); a few -0.0 among them (an fp32 add of -0.0 onto a +0.0 residual is
    +0.0: an add, not a copy)."""
    gen = torch.Generator().manual_seed(1000 + 17 * rank_id + t)
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


def _check_mask(mask):
    """Some tensors compressed, some not; among the uncompressed ones (the flat plan, in tensor
    order, dense) one at an odd flat offset and one of several flat items with a ragged tail."""
    assert any(mask) and not all(mask), mask
    unc = [n for n, c in zip(NUMEL, mask) if not c]
    offs = [sum(unc[:i]) for i in range(len(unc))]
    assert any(o % 2 == 1 for o in offs), offs
    assert any(n > FLAT_ITEM and n % FLAT_ITEM != 0 for n in unc), unc


class _Rank:
    """One process of the group: PSGD_COMM=ipc, a gloo group over a file store, cuda:0."""

    def __init__(self, rank_id, world, initfile, env=None):
        os.environ["PSGD_COMM"] = "ipc"
        os.environ.update(env or {})
        self.rank_id, self.world = rank_id, world
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=world)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def aggregator(self, rank, iters, fused):
        from powersgd_amd import Config, Fp32ResidualPowerSGD

        agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=BF16, device=self.dev) for s in SHAPES],
                                   Config(rank, _mcr(rank, iters), iters, 0), fused=fused)
        _check_mask(agg.is_compressed_mask)
        return agg

    def flow(self, rank, iters, odd, fused, steps=STEPS):
        """`steps` steps of one aggregator (one exchange session); per step the raw bits of
        everything observable."""
        agg = self.aggregator(rank, iters, fused)
        codec = agg.inner._powersgd
        rec = []
        for t in range(steps):
            grads = _place(_fresh(t, self.rank_id), odd, self.dev)
            folds = agg.fused_folds()
            final = codec._plan.fused_final(codec.step_counter, False)  # this step's final pass at W > 1
            out = agg.aggregate(grads)
            torch.cuda.synchronize()
            rec.append({
                "folds": folds,
                "final": final,
                "out": [_bits(o).cpu() for o in out],
                "residual": _bits(agg.residual).cpu(),
                "ps": _bits(codec._ps_buffer).cpu(),
                "qs": _bits(codec._qs_buffer).cpu(),
                "grads_zero": all(not bool(_bits(g).any()) for g in grads),
            })
            assert agg.step_counter == t + 1
        assert codec._ipc_open
        assert not codec.ipc_status(), "a device-side exchange wait timed out"
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
    return os.path.join(str(tmp_path), "init")


# ------------------------------------------------------------------ tests 1 and 3
def _bitwise(rank_id, world, initfile, cases, want_finals):
    me = _Rank(rank_id, world, initfile)
    finals = set()
    try:
        for rank, iters, odd in cases:
            ctx = (world, rank_id, rank, iters, odd)
            ref = me.flow(rank, iters, odd, False)  # the reference: computed once, never modified
            assert [r["folds"] for r in ref] == [(0, 0)] * STEPS, ctx  # fused=False never folds
            one = me.flow(rank, iters, odd, True)
            assert [r["folds"] for r in one] == [(0, 1)] * STEPS, (ctx, [r["folds"] for r in one])
            _same(one, ref, ctx)
            two = me.flow(rank, iters, odd, True)
            _same(two, one, (ctx, "second fused run"))
            assert any(bool(r["residual"].any()) for r in one), ctx  # the residuals are non-trivial
            finals |= {(rank, r["final"]) for r in one}
        # both output passes were reached: the apply pass and the one after a fused k_final_odd
        assert want_finals <= finals, finals
    finally:
        me.close()


@pytest.mark.parametrize("world", [2, 3])
def test_fused_equals_three_stage_flow_bitwise(world, tmp_path):
    """Test 1: bit for bit at W = 2 and W = 3 with distinct per-rank gradients, rank buckets
    1 / 2 / 4, 1-3 iterations, the placement alternating, three steps each."""
    finals = {(1, 0), (2, 0), (4, 0), (1, 1), (2, 1)}
    torch.multiprocessing.spawn(_bitwise, args=(world, _init(tmp_path), CASES, finals), nprocs=world, join=True)


def test_one_rank_group_bitwise(tmp_path):
    """Test 3: a 1-rank group over IPC takes the world-size-1 k_apply_mix (and, after a fused
    k_final_odd, k_lowrank_mix) as final pass: fused against three-stage at ranks 1 and 4."""
    cases = [(1, 1, False), (1, 2, True), (4, 1, True), (4, 2, False)]
    torch.multiprocessing.spawn(_bitwise, args=(1, _init(tmp_path), cases, {(1, 0), (4, 0), (1, 1)}), nprocs=1,
                                join=True)


# ------------------------------------------------------------------ test 2
def _agree(rank_id, world, initfile):
    me = _Rank(rank_id, world, initfile)
    try:
        for rank, iters, odd in [(1, 2, True), (2, 1, True), (4, 3, True), (2, 2, False)]:
            ctx = (rank_id, rank, iters, odd)
            rec = me.flow(rank, iters, odd, True)
            assert [r["folds"] for r in rec] == [(0, 1)] * STEPS, ctx
            mine = {"out": [r["out"] for r in rec], "residual": rec[-1]["residual"]}
            every = [None] * world
            torch.distributed.all_gather_object(every, mine)
            for w, other in enumerate(every):
                for t in range(STEPS):
                    for i, (p, q) in enumerate(zip(mine["out"][t], other["out"][t])):
                        assert torch.equal(p, q), (ctx, w, t, i, "the averages are the same on every rank")
            # every rank keeps the error of ITS gradients: a swapped local / averaged term set
            # would leave the same residual everywhere
            assert not torch.equal(every[0]["residual"], every[1]["residual"]), ctx
    finally:
        me.close()


def test_ranks_agree_on_outputs_and_differ_in_residuals(tmp_path):
    """Test 2: within a case the bf16 outputs are bit-identical across ranks, the residuals of rank
    0 and rank 1 differ."""
    torch.multiprocessing.spawn(_agree, args=(2, _init(tmp_path)), nprocs=2, join=True)


# ------------------------------------------------------------------ test 4
PLACEMENTS = ("separate", "odd", "mod4")


def _layout(placement: str):
    """Element offsets of the views in the bucket-like buffer, and its length (the layout of
    tests/test_gpu_mixed_comm_dst.py)."""
    want, mod = (1, 2) if placement == "odd" else (2, 4)
    off, offs = 8, []
    for n in NUMEL:
        gap = next(g for g in (1, 2, 3, 4) if (off + g) % mod == want)
        assert gap <= 3 or (placement == "mod4" and off % 4 == 2), (placement, off, gap)
        off += gap
        offs.append(off)
        off += n
    return offs, off + 8


class _Dst:
    """One destination set. `flat` (placements odd, mod4): the bucket-like buffer, canary everywhere."""

    def __init__(self, placement: str, dev):
        self.flat, self.offs = None, None
        if placement == "separate":
            self.views = [torch.empty(s, dtype=BF16, device=dev) for s in SHAPES]
            for v in self.views:
                v.view(torch.int16).fill_(CANARY)
            return
        self.offs, total = _layout(placement)
        self.flat = torch.empty(total, dtype=BF16, device=dev)
        self.flat.view(torch.int16).fill_(CANARY)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[o:o + n].view(s) for o, n, s in zip(self.offs, NUMEL, SHAPES)]
        for v in self.views:
            assert v.data_ptr() % 4 == 2 if placement == "odd" else v.data_ptr() % 8 == 4
        self.outside = torch.ones(total, dtype=torch.bool, device=dev)
        for o, n in zip(self.offs, NUMEL):
            self.outside[o:o + n] = False
        assert bool(self.outside[:8].all()) and bool(self.outside[-8:].all())

    def canary_intact(self) -> bool:
        if self.flat is None:
            return True
        return bool((self.flat.view(torch.int16)[self.outside] == CANARY).all())


class _DstRank(_Rank):
    def codec(self, rank, iters):
        """An fp32 residual (flat + views) and the PowerSGD over its views."""
        from powersgd_amd import Config, PowerSGD

        residual = torch.zeros(sum(NUMEL), dtype=torch.float32, device=self.dev)
        views, off = [], 0
        for s, n in zip(SHAPES, NUMEL):
            views.append(residual[off:off + n].view(s))
            off += n
        inner = PowerSGD(views, Config(rank, _mcr(rank, iters), iters, 0))
        _check_mask(inner.is_compressed_mask)
        return residual, views, inner

    def _record(self, inner, residual, dst):
        torch.cuda.synchronize()
        codec = inner._powersgd
        return {"dst": [_bits(d).cpu() for d in dst], "residual": _bits(residual).cpu(),
                "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu()}

    def _finish(self, inner):
        assert inner._powersgd._ipc_open and not inner._powersgd.ipc_status()
        inner.close()

    def reference(self, rank, iters):
        """The defining sequence: residual += float(g) (what the hook's per-bucket ADD leaves),
        psgd_aggregate_ipc on the residual into an fp32 slab (``PowerSGD.aggregate`` under
        PSGD_COMM=ipc), then the run-table GATHER of the fp32 averages into a dense bf16 buffer."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        residual, views, inner = self.codec(rank, iters)
        n = len(SHAPES)
        offs = [sum(NUMEL[:i]) for i in range(n)]
        gather = _lib.Runs(offs, list(range(n)), [0] * n, NUMEL, n, _lib.PSGD_F32, _lib.PSGD_BF16)
        ws = torch.empty(gather.workspace_bytes(), dtype=torch.uint8, device=self.dev)
        gather.bind(0, ws.data_ptr())
        out_ptrs = _lib.ptr_array([0] * n)
        rec = []
        for t in range(STEPS):
            for v, g in zip(views, _fresh(t, self.rank_id)):
                v.add_(g.to(self.dev).float())
            avg = inner.aggregate(views)
            _psgd_host.fill_list(avg, ctypes.addressof(out_ptrs), _lib.PSGD_F32, 0)
            bucket = torch.empty(sum(NUMEL), dtype=BF16, device=self.dev)
            bucket.view(torch.int16).fill_(CANARY)
            gather.gather(bucket.data_ptr(), ctypes.addressof(out_ptrs), self.stream)
            rec.append(self._record(inner, residual, [bucket[o:o + k] for o, k in zip(offs, NUMEL)]))
        self._finish(inner)
        return rec

    def fused(self, rank, iters, placement):
        """The direct call with PowerSGD.aggregate's bookkeeping (both step counters, the split by
        the compression mask, the exchange set up once), as the DDP hook makes it."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        residual, views, inner = self.codec(rank, iters)
        codec = inner._powersgd
        assert codec._plan.mixed_folds_dst(0, self.world) == 1 and codec._plan.mixed_folds_dst(1, self.world) == 1
        dst = _Dst(placement, self.dev)
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, _lib.PSGD_BF16, 0)
        codec._ipc_setup(inner._unc.numel)
        rec = []
        for t in range(STEPS):
            for v, g in zip(views, _fresh(t, self.rank_id)):
                v.add_(g.to(self.dev).float())
            table.fill(dst.views)
            inner.step_counter += 1
            inner._table.fill(views)
            codec._plan.aggregate_mixed_ipc_dst(inner._table.comp_addr(), table.comp_addr(), codec.step_counter,
                                                self.stream, flat=inner._unc.plan,
                                                unc_residual=inner._table.unc_addr(), unc_dst_bf16=table.unc_addr())
            codec.step_counter += 1
            r = self._record(inner, residual, [d.reshape(-1) for d in dst.views])
            r["canary"] = dst.canary_intact()
            rec.append(r)
        self._finish(inner)
        return rec


def _same_dst(a, b, ctx):
    for t, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x["dst"], y["dst"])):
            assert torch.equal(p, q), (ctx, t, i, "destination")
        for k in ("residual", "ps", "qs"):
            assert torch.equal(x[k], y[k]), (ctx, t, k)


def _dst_bitwise(rank_id, world, initfile):
    me = _DstRank(rank_id, world, initfile)
    try:
        for rank in (1, 2, 4):
            for iters in (1, 2):
                ref = me.reference(rank, iters)  # once per case, shared by the placements, never modified
                assert any(bool(r["residual"].any()) for r in ref)
                for placement in PLACEMENTS:
                    ctx = (world, rank_id, rank, iters, placement)
                    one = me.fused(rank, iters, placement)
                    _same_dst(one, ref, ctx)
                    assert all(r["canary"] for r in one), (ctx, [r["canary"] for r in one])
                    if placement == "odd":  # (the run-to-run check needs no second placement)
                        two = me.fused(rank, iters, placement)
                        _same_dst(two, one, (ctx, "second fused run"))
    finally:
        me.close()


def test_dst_form_equals_reference_sequence_bitwise(tmp_path):
    """Test 4: psgd_aggregate_mixed_ipc_dst at W = 2 (real processes, distinct gradients) against
    psgd_aggregate_ipc into an fp32 slab followed by the run-table GATHER: rank buckets 1 / 2 / 4,
    1-2 iterations, three destination placements with canaries between and around the views."""
    torch.multiprocessing.spawn(_dst_bitwise, args=(2, _init(tmp_path)), nprocs=2, join=True)


# ------------------------------------------------------------------ test 5
def _refusals(rank_id, initfile):
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    me = _Rank(0, 1, initfile)
    try:
        dev = me.dev
        shapes = [(300, 520), (130, 67)]
        numel = sum(torch.Size(s).numel() for s in shapes)

        def state(codec):
            gen = torch.Generator().manual_seed(5)
            grads = [torch.randn(s, generator=gen).to(BF16).to(dev) for s in shapes]
            resid = [torch.randn(s, generator=gen).to(dev) for s in shapes]
            out = torch.full((numel,), 3.0, dtype=BF16, device=dev)
            dst = [torch.full(s, 3.0, dtype=BF16, device=dev) for s in shapes]
            return grads, resid, out, dst, grads + resid + dst + [out, codec._ps_buffer, codec._qs_buffer]

        def calls(codec, grads, resid, out, dst):
            gp = _lib.ptr_array([g.data_ptr() for g in grads])
            rp = _lib.ptr_array([r.data_ptr() for r in resid])
            dp = _lib.ptr_array([d.data_ptr() for d in dst])
            plan = codec._plan
            return ((gp, rp, dp),
                    lambda: plan.aggregate_mixed_ipc(ctypes.addressof(gp), ctypes.addressof(rp), out.data_ptr(), 0,
                                                     me.stream),
                    lambda: plan.aggregate_mixed_ipc_dst(ctypes.addressof(rp), ctypes.addressof(dp), 0, me.stream))

        def unchanged(live, keep, ctx):
            torch.cuda.synchronize()
            for a, b in zip(live, keep):
                assert torch.equal(_bits(a) if a.dtype == BF16 else a, _bits(b) if b.dtype == BF16 else b), ctx

        def f32_codec():
            return BasicPowerSGD([torch.zeros(s, device=dev) for s in shapes], BasicConfig(2, 2))

        # the open 1-rank session the refusals must leave usable
        good = f32_codec()
        good._ipc_setup(0)
        assert good._plan.mixed_folds_comm(0, 1) == (0, 1) and good._plan.mixed_folds_dst(0, 1) == 1

        for what in ("rank8", "bf16", "wide"):
            rank = {"rank8": 8, "bf16": 2, "wide": 64}[what]
            dt = BF16 if what == "bf16" else torch.float32
            codec = BasicPowerSGD([torch.zeros(s, dtype=dt, device=dev) for s in shapes], BasicConfig(rank, 2))
            assert codec._plan.is_wide() == (what == "wide")
            if what != "wide":  # (the exchange itself refuses wide plans: no session to open)
                codec._ipc_setup(0)
            grads, resid, out, dst, live = state(codec)
            keep = [x.clone() for x in live]
            _, dense, to_dst = calls(codec, grads, resid, out, dst)
            for call in (dense, to_dst):
                with pytest.raises(ValueError, match="psgd_aggregate_mixed"):  # PSGD_ERR_VALUE
                    call()
                unchanged(live, keep, what)
            codec.close()

        # an eligible plan without an open session: PSGD_ERR_STATE
        closed = f32_codec()
        grads, resid, out, dst, live = state(closed)
        keep = [x.clone() for x in live]
        _, dense, to_dst = calls(closed, grads, resid, out, dst)
        for call in (dense, to_dst):
            with pytest.raises(RuntimeError, match="STATE.*psgd_ipc_open first"):
                call()
            unchanged(live, keep, "no session")

        # the reference of the eligible call: the ADD, psgd_aggregate_ipc into an fp32 slab on a
        # session of its own, the bf16 rounding (round to nearest even, as the run-table GATHER)
        ref = f32_codec()
        ref._ipc_setup(0)
        grads, resid, _, _, _ = state(ref)
        for r, g in zip(resid, grads):
            r.add_(g.float())
        rp = _lib.ptr_array([r.data_ptr() for r in resid])
        slab = torch.zeros(numel, device=dev)
        ref._plan.aggregate_ipc(ctypes.addressof(rp), slab.data_ptr(), 0, None, None, 0, me.stream)
        torch.cuda.synchronize()
        want = {"out": _bits(slab.to(BF16)).cpu(), "resid": [r.clone() for r in resid], "ps": ref._ps_buffer.clone(),
                "qs": ref._qs_buffer.clone()}
        ref.close()

        # the next eligible calls on the session that was open all along succeed and match it
        grads, resid, out, dst, _ = state(good)
        keep_alive, dense, _ = calls(good, grads, resid, out, dst)
        dense()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out).cpu(), want["out"])
        assert all(torch.equal(a, b) for a, b in zip(resid, want["resid"]))
        assert torch.equal(good._ps_buffer, want["ps"]) and torch.equal(good._qs_buffer, want["qs"])
        assert all(not bool(_bits(g).any()) for g in grads)
        assert not good.ipc_status()
        good.close()

        good = f32_codec()
        good._ipc_setup(0)
        grads, resid, out, dst, _ = state(good)
        for r, g in zip(resid, grads):  # the _dst form runs no ADD: the residual already holds the sum
            r.add_(g.float())
        keep_alive, _, to_dst = calls(good, grads, resid, out, dst)
        to_dst()
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([_bits(d).reshape(-1) for d in dst]).cpu(), want["out"])
        assert all(torch.equal(a, b) for a, b in zip(resid, want["resid"]))
        assert torch.equal(good._ps_buffer, want["ps"]) and torch.equal(good._qs_buffer, want["qs"])
        assert not good.ipc_status()
        good.close()
    finally:
        me.close()


def test_refusals_touch_nothing(tmp_path):
    """Test 5: rank bucket 8, a bf16 plan and a wide plan return PSGD_ERR_VALUE from both entries,
    an eligible plan without a session PSGD_ERR_STATE; gradients, residual, destinations and P/Q stay
    bit-identical, and the next eligible call on the open session matches the reference."""
    torch.multiprocessing.spawn(_refusals, args=(_init(tmp_path),), nprocs=1, join=True)


# ------------------------------------------------------------------ test 6
def _give_up(rank_id, initfile):
    me = _Rank(rank_id, 2, initfile, {"PSGD_IPC_SPIN": "4000"})  # ~1 ms of polling
    try:
        agg = me.aggregator(2, 2, True)
        codec = agg.inner._powersgd
        codec._ipc_setup(agg.inner._unc.numel)  # collective: both ranks
        if rank_id == 0:  # rank 1 never takes the step: rank 0's waits give up by themselves, no hang
            assert agg.fused_folds() == (0, 1)
            out = agg.aggregate(_place(_fresh(0, 0), False, me.dev))
            torch.cuda.synchronize()
            # invalid sums come back as NaN, never as plausible stale values: the compressed
            # tensors' averages and every element of the uncompressed tensors' (k_xchg_mix)
            for o, c in zip(out, agg.is_compressed_mask):
                nan = torch.isnan(o.float())
                assert bool(nan.any()) if c else bool(nan.all()), (tuple(o.shape), c)
            assert codec.ipc_status()
            # the next fused step is refused before the ADD: the gradients are not consumed
            grads = _place(_fresh(1, 0), True, me.dev)
            keep = [_bits(g).clone() for g in grads]
            resid = _bits(agg.residual).clone()
            with pytest.raises(RuntimeError, match="timed out"):
                agg.aggregate(grads)
            torch.cuda.synchronize()
            assert all(torch.equal(_bits(g), k) for g, k in zip(grads, keep))
            assert torch.equal(_bits(agg.residual), resid)
        agg.close()
        assert not codec.ipc_status()
    finally:
        me.close()


def test_fused_wait_is_bounded():
    """Test 6: the exchange's designed give-up path under the fused step, as test_ipc_wait_is_bounded
    (tests/test_gpu_ipc.py) for the plain one: run once."""
    import tempfile

    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_give_up, args=(os.path.join(td, "init"),), nprocs=2, join=True)
