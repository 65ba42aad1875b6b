"""psgd_aggregate_ipc_dst (the default fp32 DDP hook's one-call completion under ``PSGD_COMM=ipc``)
against the sequence it is defined as on the same build: psgd_aggregate_ipc (``PowerSGD.aggregate``
of the gradient views under PSGD_COMM=ipc) followed by a plain copy of every average to its
destination.

Defined as that sequence, so there is no tolerance: ``torch.equal`` on raw bits, after every step
and on every rank, of every destination, the residual and the codec's ``_ps_buffer`` /
``_qs_buffer``.

World size 2 is two real processes on cuda:0 (``torch.multiprocessing.spawn``, a gloo group over a
file store, as tests/test_gpu_mixed_ipc.py), and every rank holds its OWN gradients (the seed
includes the rank): the local and the averaged factors differ. Shapes, min_compression_rate, the
destination placements and the NaN-pattern canaries are those of tests/test_gpu_comm_dst.py, plus
``(2049,)``: an uncompressed tensor of more than kFlatItem = 2048 elements with a ragged tail (two
copy items, the second of one element)."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(128, 64, 3, 3), (256, 300), (96, 200), (64, 100), (50, 150), (33, 65), (7, 5), (2049,), (40,), (97,), (1,)]
NUMEL = [torch.Size(s).numel() for s in SHAPES]
STEPS = 3
CANARY = 0x7FC12345  # a quiet NaN with a payload: no average is a NaN
PLACEMENTS = {"aligned": 0, "one_in": 1, "two_in": 2}
CASES = [(rank, iters) for rank in (1, 4, 16) for iters in (1, 2)]


def _rate(shape, rank, iters):
    sh = list(shape)
    return torch.Size(sh).numel() / (0.5 * iters * min(rank, min(sh)) * sum(sh))


def _mcr(rank, iters):
    # 0.99 x the smallest rate of a 2-D shape: every 2-D shape compresses, a 1-D tensor of more than
    # one element (rate 2 / (I min(r, numel))) never does
    return 0.99 * min(_rate(s, rank, iters) for s in SHAPES if len(s) > 1)


def _fresh(t, rank_id):
    """Seeded gradients of step t on rank `rank_id` (every rank its own), growing in scale; a few -0.0."""
    gen = torch.Generator().manual_seed(3000 + 17 * rank_id + t)
    out = []
    for s in SHAPES:
        g = torch.randn(s, generator=gen) * float(2 ** t)
        g.view(-1)[::7] = -0.0
        out.append(g)
    return out


def _layout(want):
    off, offs = 8, []
    for n in NUMEL:
        off += next(g for g in (1, 2, 3, 4) if (off + g) % 4 == want)
        offs.append(off)
        off += n
    return offs, off + 8


class _Dst:
    """One destination set: a bucket-like buffer, every view at offset % 4 == want, canary elsewhere."""

    def __init__(self, placement, dev):
        want = PLACEMENTS[placement]
        self.offs, total = _layout(want)
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat.view(torch.int32).fill_(CANARY)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[o:o + n].view(s) for o, n, s in zip(self.offs, NUMEL, SHAPES)]
        assert all(v.data_ptr() % 16 == 4 * want for v in self.views)
        self.outside = torch.ones(total, dtype=torch.bool, device=dev)
        for o, n in zip(self.offs, NUMEL):
            self.outside[o:o + n] = False

    def canary_intact(self):
        return bool((self.flat.view(torch.int32)[self.outside] == CANARY).all())


def _bits(x):
    return x.contiguous().view(torch.int32)


class _Rank:
    """One process of the group: PSGD_COMM=ipc, a gloo group over a file store, cuda:0."""

    def __init__(self, rank_id, world, initfile):
        os.environ["PSGD_COMM"] = "ipc"
        self.rank_id, self.world = rank_id, world
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=world)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def codec(self, rank, iters):
        from powersgd_amd import Config, PowerSGD

        grads = torch.zeros(sum(NUMEL), dtype=torch.float32, device=self.dev)
        views, off = [], 0
        for s, n in zip(SHAPES, NUMEL):
            views.append(grads[off:off + n].view(s))
            off += n
        inner = PowerSGD(views, Config(rank, _mcr(rank, iters), iters, 0))
        mask = inner.is_compressed_mask
        assert all(mask[:7]) and not any(mask[7:10]), (rank, iters, mask)
        return grads, views, inner

    def _record(self, inner, grads, final, dst):
        torch.cuda.synchronize()
        codec = inner._powersgd
        return {"final": final, "dst": [_bits(d).cpu() for d in dst], "residual": _bits(grads).cpu(),
                "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu()}

    def _finish(self, inner):
        assert inner._powersgd._ipc_open and not inner._powersgd.ipc_status()
        inner.close()

    def reference(self, rank, iters):
        """The defining sequence: psgd_aggregate_ipc into the output slab, then a plain copy."""
        grads, views, inner = self.codec(rank, iters)
        rec = []
        for t in range(STEPS):
            for v, g in zip(views, _fresh(t, self.rank_id)):
                v.add_(g.to(self.dev))
            codec = inner._powersgd
            final = codec._plan.fused_final(codec.step_counter, False)
            avg = inner.aggregate(views)
            rec.append(self._record(inner, grads, final, [a.clone().reshape(-1) for a in avg]))
        self._finish(inner)
        return rec

    def direct(self, rank, iters, placement):
        """The one call with PowerSGD.aggregate's bookkeeping (both step counters, the split by the
        compression mask, the exchange set up once), as the DDP hook makes it."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        grads, views, inner = self.codec(rank, iters)
        codec = inner._powersgd
        assert codec._plan.dst_ok(0, self.world) == 1 and codec._plan.dst_ok(1, self.world) == 1
        dst = _Dst(placement, self.dev)
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, _lib.PSGD_F32, 0)
        codec._ipc_setup(inner._unc.numel)
        rec = []
        for t in range(STEPS):
            for v, g in zip(views, _fresh(t, self.rank_id)):
                v.add_(g.to(self.dev))
            final = codec._plan.fused_final(codec.step_counter, False)
            table.fill(dst.views)
            inner.step_counter += 1
            inner._table.fill(views)
            codec._plan.aggregate_ipc_dst(inner._table.comp_addr(), table.comp_addr(), codec.step_counter, self.stream,
                                          flat=inner._unc.plan, unc=inner._table.unc_addr(), unc_dst=table.unc_addr())
            codec.step_counter += 1
            r = self._record(inner, grads, final, [d.reshape(-1) for d in dst.views])
            r["canary"] = dst.canary_intact()
            rec.append(r)
        self._finish(inner)
        return rec

    def close(self):
        torch.distributed.destroy_process_group()


def _same(a, b, ctx):
    for t, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x["dst"], y["dst"])):
            assert torch.equal(p, q), (ctx, t, i, "destination")
        for k in ("residual", "ps", "qs"):
            assert torch.equal(x[k], y[k]), (ctx, t, k)


def _init(tmp_path):
    return os.path.join(str(tmp_path), "init")


def _bitwise(rank_id, world, initfile):
    me = _Rank(rank_id, world, initfile)
    finals = set()
    try:
        for rank, iters in CASES:
            ref = me.reference(rank, iters)  # once per case, shared by the placements, never modified
            assert any(bool(r["residual"].any()) for r in ref)
            for placement in PLACEMENTS:
                ctx = (world, rank_id, rank, iters, placement)
                one = me.direct(rank, iters, placement)
                _same(one, ref, ctx)
                assert all(r["canary"] for r in one), (ctx, [r["canary"] for r in one])
                finals |= {(rank, r["final"]) for r in one}
            # every rank keeps the error of ITS gradients, the averages agree
            mine = {"dst": ref[-1]["dst"], "residual": ref[-1]["residual"]}
            every = [None] * world
            torch.distributed.all_gather_object(every, mine)
            assert all(torch.equal(p, q) for p, q in zip(every[0]["dst"], every[1]["dst"])), (rank, iters)
            assert not torch.equal(every[0]["residual"], every[1]["residual"]), (rank, iters)
        # both output passes were reached: the apply pass and the one after a fused k_final_odd
        assert {(1, 0), (4, 0), (16, 0), (1, 1)} <= finals, finals
    finally:
        me.close()


def test_ipc_dst_equals_reference_sequence_bitwise(tmp_path):
    """Two processes on one GPU, distinct gradients per rank: rank buckets 1, 4 and 16, 1-2
    iterations, three placements with canaries around the views, three steps each."""
    torch.multiprocessing.spawn(_bitwise, args=(2, _init(tmp_path)), nprocs=2, join=True)


def _refusals(rank_id, initfile):
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    me = _Rank(0, 1, initfile)
    try:
        dev = me.dev
        shapes = [(96, 200), (33, 65)]
        numel = sum(torch.Size(s).numel() for s in shapes)

        def codec_():
            return BasicPowerSGD([torch.zeros(s, device=dev) for s in shapes], BasicConfig(2, 2))

        def state(codec):
            gen = torch.Generator().manual_seed(5)
            grads = [torch.randn(s, generator=gen).to(dev) for s in shapes]
            dst = [torch.full(s, 3.0, device=dev) for s in shapes]
            return grads, dst, grads + dst + [codec._ps_buffer, codec._qs_buffer]

        def call(codec, grads, dst):
            gp = _lib.ptr_array([g.data_ptr() for g in grads])
            dp = _lib.ptr_array([d.data_ptr() for d in dst])
            codec._plan.aggregate_ipc_dst(ctypes.addressof(gp), ctypes.addressof(dp), 0, me.stream)

        # an eligible plan without an open session: PSGD_ERR_STATE, nothing touched
        closed = codec_()
        assert closed._plan.dst_ok(0, 1) == 1
        grads, dst, live = state(closed)
        keep = [x.clone() for x in live]
        with pytest.raises(RuntimeError, match="STATE.*psgd_ipc_open first"):
            call(closed, grads, dst)
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(live, keep))

        # the reference of the eligible call: psgd_aggregate_ipc into a slab on a session of its own
        ref = codec_()
        ref._ipc_setup(0)
        rgrads, _, _ = state(ref)
        rp = _lib.ptr_array([g.data_ptr() for g in rgrads])
        slab = torch.zeros(numel, device=dev)
        ref._plan.aggregate_ipc(ctypes.addressof(rp), slab.data_ptr(), 0, None, None, 0, me.stream)
        torch.cuda.synchronize()
        want_ps, want_qs = ref._ps_buffer.clone(), ref._qs_buffer.clone()
        ref.close()

        # the refused plan's next session is usable and matches it
        closed._ipc_setup(0)
        call(closed, grads, dst)
        torch.cuda.synchronize()
        assert torch.equal(_bits(torch.cat([d.reshape(-1) for d in dst])), _bits(slab))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, rgrads))
        assert torch.equal(closed._ps_buffer, want_ps) and torch.equal(closed._qs_buffer, want_qs)
        assert not closed.ipc_status()
        closed.close()
    finally:
        me.close()


def test_refusal_without_a_session_touches_nothing(tmp_path):
    """No open session: PSGD_ERR_STATE before anything is launched; gradients, destinations and P/Q
    stay bit-identical, and the plan's next session runs the call and matches psgd_aggregate_ipc."""
    torch.multiprocessing.spawn(_refusals, args=(_init(tmp_path),), nprocs=1, join=True)
