"""psgd_aggregate_comm_dst (the default fp32 DDP hook's one-call completion: the final pass of
the communicator sequence stores each tensor's fp32 average at the tensor's own destination)
against the sequence it is defined as, on the same build and the same communicator:
psgd_aggregate_comm (``PowerSGD.aggregate`` of the gradient views) followed by a plain copy of every
average to its destination.

Defined as that sequence, so there is no tolerance: ``torch.equal`` on raw bits, after every step,
of every destination, the residual and the codec's ``_ps_buffer`` / ``_qs_buffer``, and the
stand-in's collective count per step.

World size W runs on ONE GPU through the stand-in collective library (tests/stubs/rccl_stub.hip),
set up as tests/test_gpu_mixed_comm_dst.py does. The shapes are the smallest that reach every store
path: m % 64 != 0 and m % 4 != 0 under the matrix-core tiles, the scalar layout, an effective rank
below its bucket, a row count that is no multiple of a tile's chunk, odd-length uncompressed
tensors. min_compression_rate is 0.99 x the smallest rate of a 2-D shape (numel / (0.5 I min(r,
min(shape)) sum(shape)), the codec's rule), so every 2-D shape compresses; (40,) and (97,) never do
(their rate is 2 / (I min(r, numel))), (1,) does from rank bucket 4 on (rate 2 / I).

All destinations live in one bucket-like buffer, in three placements: every view 16-byte aligned;
every view one element in (4-byte aligned only); every view two elements in (8-byte aligned). Every
element outside the views (8 before the first and after the last, 1-4 between neighbours) holds a
NaN-pattern canary that must survive every step: a store past a tensor would land on its bucket
neighbour."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
SHAPES = [(128, 64, 3, 3), (256, 300), (96, 200), (64, 100), (50, 150), (33, 65), (7, 5), (40,), (97,), (1,)]
NUMEL = [torch.Size(s).numel() for s in SHAPES]
STEPS = 4
ITERS = (1, 2, 3)
CANARY = 0x7FC12345  # a quiet NaN with a payload: no average is a NaN
PLACEMENTS = {"aligned": 0, "one_in": 1, "two_in": 2}


def _rate(shape, rank, iters):
    sh = list(shape)
    numel = torch.Size(sh).numel()
    return numel / (0.5 * iters * min(rank, min(sh)) * sum(sh))


def _mcr(rank, iters):
    return 0.99 * min(_rate(s, rank, iters) for s in SHAPES if len(s) > 1)


def _fresh(t):
    """Seeded gradients of step t whose scale grows each step (non-trivial residuals); a few -0.0."""
    gen = torch.Generator().manual_seed(2000 + t)
    out = []
    for s in SHAPES:
        g = torch.randn(s, generator=gen) * float(2 ** t)
        g.view(-1)[::7] = -0.0
        out.append(g)
    return out


def _layout(want):
    """Element offsets of the views (offset % 4 == want) in the bucket-like buffer, and its length."""
    off, offs = 8, []
    for n in NUMEL:
        off += next(g for g in (1, 2, 3, 4) if (off + g) % 4 == want)
        offs.append(off)
        off += n
    return offs, off + 8


class _Dst:
    """One destination set: the bucket-like buffer, canary everywhere."""

    def __init__(self, placement, dev):
        want = PLACEMENTS[placement]
        self.offs, total = _layout(want)
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat.view(torch.int32).fill_(CANARY)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[o:o + n].view(s) for o, n, s in zip(self.offs, NUMEL, SHAPES)]
        for v in self.views:
            assert v.data_ptr() % 16 == 4 * want
        self.outside = torch.ones(total, dtype=torch.bool, device=dev)
        for o, n in zip(self.offs, NUMEL):
            self.outside[o:o + n] = False
        assert bool(self.outside[:8].all()) and bool(self.outside[-8:].all())
        assert all(bool(self.outside[o - 1]) and bool(self.outside[o + n]) for o, n in zip(self.offs, NUMEL))

    def canary_intact(self):
        return bool((self.flat.view(torch.int32)[self.outside] == CANARY).all())


def _bits(x):
    return x.contiguous().view(torch.int32)


class _Child:
    """The child's side of a case: the stub as the library's collective library, a one-rank gloo
    group (it only makes is_distributed() true), communicators of world `world`."""

    def __init__(self, init, world):
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
        self.world = world
        self.stub = ctypes.CDLL(STUB)  # the same handle the library opened: one call counter
        self.stub.psgd_stub_calls.restype = ctypes.c_longlong
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def comm(self):
        from powersgd_amd import _lib

        return _lib.Comm(self.world, 0, _lib.comm_unique_id(), 0)

    def codec(self, rank, iters):
        """The gradient buffer (flat + views) and the PowerSGD over its views, on a fresh communicator."""
        from powersgd_amd import Config, PowerSGD

        grads = torch.zeros(sum(NUMEL), dtype=torch.float32, device=self.dev)
        views, off = [], 0
        for s, n in zip(SHAPES, NUMEL):
            views.append(grads[off:off + n].view(s))
            off += n
        inner = PowerSGD(views, Config(rank, _mcr(rank, iters), iters, 0))
        inner._powersgd._comm = self.comm()
        mask = inner.is_compressed_mask
        assert all(mask[:7]) and not mask[7] and not mask[8], (rank, iters, mask)
        return grads, views, inner

    def _record(self, inner, grads, calls, final, dst):
        torch.cuda.synchronize()
        codec = inner._powersgd
        return {"calls": calls, "final": final, "dst": [_bits(d).cpu() for d in dst],
                "residual": _bits(grads).cpu(), "ps": _bits(codec._ps_buffer).cpu(),
                "qs": _bits(codec._qs_buffer).cpu()}

    def reference(self, rank, iters, steps=STEPS):
        """The defining sequence: psgd_aggregate_comm on the gradients (which the hook's per-bucket ADD
        accumulated into the residual), then a plain copy of every average."""
        grads, views, inner = self.codec(rank, iters)
        rec = []
        for t in range(steps):
            for v, g in zip(views, _fresh(t)):
                v.add_(g.to(self.dev))
            codec = inner._powersgd
            final = codec._plan.fused_final(codec.step_counter, False)
            n0 = self.stub.psgd_stub_calls()
            avg = inner.aggregate(views)
            dst = [a.clone().reshape(-1) for a in avg]
            rec.append(self._record(inner, grads, self.stub.psgd_stub_calls() - n0, final, dst))
        inner.close()
        return rec

    def direct(self, rank, iters, placement, steps=STEPS):
        """The one call with PowerSGD.aggregate's bookkeeping (both step counters, the split by the
        compression mask), as the DDP hook makes it."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        grads, views, inner = self.codec(rank, iters)
        codec = inner._powersgd
        assert codec._plan.dst_ok(0, self.world) == codec._plan.dst_ok(1, self.world)
        if codec._plan.dst_ok(0, self.world) != 1:
            inner.close()
            return None  # an instance this plan needs is not admitted: the plan keeps the three stages
        dst = _Dst(placement, self.dev)
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, _lib.PSGD_F32, 0)
        rec = []
        for t in range(steps):
            for v, g in zip(views, _fresh(t)):
                v.add_(g.to(self.dev))
            final = codec._plan.fused_final(codec.step_counter, False)
            n0 = self.stub.psgd_stub_calls()
            table.fill(dst.views)
            inner.step_counter += 1
            inner._table.fill(views)
            codec._plan.aggregate_comm_dst(inner._table.comp_addr(), table.comp_addr(), codec.step_counter, codec._comm,
                                           self.stream, flat=inner._unc.plan, unc=inner._table.unc_addr(),
                                           unc_dst=table.unc_addr())
            codec.step_counter += 1
            r = self._record(inner, grads, self.stub.psgd_stub_calls() - n0, final, [d.reshape(-1) for d in dst.views])
            r["canary"] = dst.canary_intact()
            rec.append(r)
        inner.close()
        return rec

    def close(self):
        torch.distributed.destroy_process_group()


def _same(a, b, ctx):
    for t, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x["dst"], y["dst"])):
            assert torch.equal(p, q), (ctx, t, i, "destination")
        for k in ("residual", "ps", "qs"):
            assert torch.equal(x[k], y[k]), (ctx, t, k)
        assert x["calls"] == y["calls"], (ctx, t, "collective count")


def _init(tmp_path):
    return f"file://{tmp_path}/store"


# Plans with a destination-table instance that keeps one wave per SIMD (profiles/ddp_direct/
# resources.txt): rank bucket 8 with two register-cached terms in two term sets
# (I = 2, W > 1) or three shared ones (I = 3, one rank). Eligibility is a property of the plan (every
# instance, both communicator kinds), so these report 0 at every world size and keep the three
# stages. Everything else must run: a plan that silently reports 0 would make the comparison vacuous.
def _not_admitted(rank, iters, world):
    return rank == 8 and iters in (2, 3)


# ------------------------------------------------------------------ test 1
def _bitwise(_, init, world, ranks):
    ch = _Child(init, world)
    finals = set()
    try:
        for rank in ranks:
            for iters in ITERS:
                ref = ch.reference(rank, iters)  # once per case, shared by the placements, never modified
                assert [r["calls"] for r in ref] == [iters + 1] * STEPS, (world, rank, iters)
                assert any(bool(r["residual"].any()) for r in ref)  # the residuals are non-trivial
                for placement in PLACEMENTS:
                    ctx = (world, rank, iters, placement)
                    one = ch.direct(rank, iters, placement)
                    if one is None:
                        assert _not_admitted(rank, iters, world), ctx
                        break
                    assert not _not_admitted(rank, iters, world), ctx
                    _same(one, ref, ctx)
                    assert all(r["canary"] for r in one), (ctx, [r["canary"] for r in one])
                    finals |= {(rank, r["final"]) for r in one}
        # both endings were reached: the apply pass (every rank bucket) and the output pass after a
        # fused k_final_odd (rank buckets 1 and 2)
        want = {(r, 0) for r in ranks} | {(r, 1) for r in ranks if r <= 2}
        assert want <= finals, (finals, want)
    finally:
        ch.close()


@pytest.mark.parametrize("ranks", [(1, 2, 4), (8, 16, 32)])
@pytest.mark.parametrize("world", [3, 4, 1])
def test_direct_call_equals_reference_sequence_bitwise(world, ranks, tmp_path):
    """Rank buckets 1-32 x 1-3 iterations x three placements x four steps, at W = 3, W = 4 and on a
    1-rank communicator."""
    torch.multiprocessing.spawn(_bitwise, args=(_init(tmp_path), world, ranks), nprocs=1, join=True)


# ------------------------------------------------------------------ test 2
def _refusals(_, init):
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    ch = _Child(init, 4)
    try:
        dev = ch.dev
        shapes = [(96, 200), (33, 65)]

        def state(codec, dt):
            gen = torch.Generator().manual_seed(5)
            grads = [torch.randn(s, generator=gen).to(dev).to(dt) for s in shapes]
            dst = [torch.full(s, 3.0, dtype=dt, device=dev) for s in shapes]
            return grads, dst, grads + dst + [codec._ps_buffer, codec._qs_buffer]

        def unchanged(live, keep, n0, ctx):
            torch.cuda.synchronize()
            for a, b in zip(live, keep):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), ctx
            assert ch.stub.psgd_stub_calls() == n0, ctx

        def call(codec, grads, dst, comm, null_table=False):
            gp = _lib.ptr_array([g.data_ptr() for g in grads])
            dp = _lib.ptr_array([d.data_ptr() for d in dst])
            codec._plan.aggregate_comm_dst(ctypes.addressof(gp), None if null_table else ctypes.addressof(dp), 0, comm,
                                           ch.stream)

        for what in ("bf16", "f64", "wide"):
            dt = {"bf16": torch.bfloat16, "f64": torch.float64, "wide": torch.float32}[what]
            torch.set_default_dtype(torch.float64 if what == "f64" else torch.float32)  # P/Q follow it
            codec = BasicPowerSGD([torch.zeros(s, dtype=dt, device=dev) for s in shapes],
                                  BasicConfig(64 if what == "wide" else 2, 2))
            torch.set_default_dtype(torch.float32)
            for w in (1, 4):
                assert codec._plan.dst_ok(0, w) == 0 and codec._plan.dst_ok(1, w) == 0
            comm = ch.comm()
            grads, dst, live = state(codec, dt)
            keep = [x.clone() for x in live]
            n0 = ch.stub.psgd_stub_calls()
            with pytest.raises(ValueError if what == "wide" else RuntimeError, match="psgd_aggregate_comm_dst"):
                call(codec, grads, dst, comm)
            unchanged(live, keep, n0, what)

        codec = BasicPowerSGD([torch.zeros(s, device=dev) for s in shapes], BasicConfig(2, 2))
        assert codec._plan.dst_ok(0, 4) == 1
        comm = ch.comm()
        grads, dst, live = state(codec, torch.float32)
        keep = [x.clone() for x in live]
        n0 = ch.stub.psgd_stub_calls()
        with pytest.raises(ValueError, match="null argument"):
            call(codec, grads, dst, comm, null_table=True)
        unchanged(live, keep, n0, "null table")
        # a null entry, and a destination that is not 4-byte aligned, likewise; neither poisons
        gp = _lib.ptr_array([g.data_ptr() for g in grads])
        for bad, exc, msg in (([dst[0].data_ptr(), 0], ValueError, "null gradient pointer"),
                              ([dst[0].data_ptr(), dst[1].data_ptr() + 2], RuntimeError, "4-byte aligned")):
            with pytest.raises(exc, match=msg):
                codec._plan.aggregate_comm_dst(ctypes.addressof(gp), ctypes.addressof(_lib.ptr_array(bad)), 0, comm,
                                               ch.stream)
            unchanged(live, keep, n0, msg)
        # a poisoned communicator (a psgd_aggregate_comm call that failed past its argument checks:
        # a null gradient pointer, refused before anything runs) is refused at entry
        f32_out = torch.zeros(sum(torch.Size(s).numel() for s in shapes), device=dev)
        bad = _lib.ptr_array([0] * len(shapes))
        with pytest.raises(ValueError, match="null gradient pointer"):
            codec._plan.aggregate_comm(ctypes.addressof(bad), f32_out.data_ptr(), 0, None, None, 0, comm, ch.stream)
        with pytest.raises(RuntimeError, match="communicator unusable"):
            call(codec, grads, dst, comm)
        unchanged(live, keep, n0, "poisoned")
        # the refusals above left a fresh communicator's plan usable
        comm2 = ch.comm()
        call(codec, grads, dst, comm2)
        torch.cuda.synchronize()
        assert not torch.equal(dst[0], keep[2])
    finally:
        ch.close()


def test_refusals_touch_nothing(tmp_path):
    """A bf16 plan, an fp64 plan and a rank-64 plan, a null table, a null entry, a misaligned
    destination and a poisoned communicator are refused before anything is launched; gradients,
    destinations, P/Q and the collective count stay."""
    torch.multiprocessing.spawn(_refusals, args=(_init(tmp_path),), nprocs=1, join=True)
