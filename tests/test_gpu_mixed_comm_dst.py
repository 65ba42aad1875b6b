"""psgd_aggregate_mixed_comm_dst (the DDP hook's one-call completion: the final pass of the
communicator sequence stores each tensor's bf16 average at the tensor's own destination) against
the sequence it is defined as, on the same build and the same communicator: psgd_aggregate_comm on
the fp32 residual (``PowerSGD.aggregate`` of the residual views) and the run-table GATHER of the
fp32 averages into bf16.

Defined as that sequence, so there is no tolerance: ``torch.equal`` on raw bits, after every step,
of the destinations, the fp32 residual and the codec's ``_ps_buffer`` / ``_qs_buffer``, and the
stand-in's collective count per step.

World size W runs on ONE GPU through the stand-in collective library (tests/stubs/rccl_stub.hip),
set up as tests/test_gpu_mixed_comm.py does; shapes, min_compression_rate and the gradient recipe
(with its -0.0 elements) are that file's. Three destination placements:
  (a) separate tensors (16-byte aligned or better);
  (b) one bucket-like flat bf16 buffer, every view at an odd element offset (2-byte aligned only);
  (c) the same with every view at an offset = 2 mod 4 elements (4-byte, not 8-byte aligned).
In (b) and (c) every element outside the views (at least 8 before the first view and after the
last, 1-3 between neighbours; in (c) 4 after a tensor whose element count is a multiple of 4, where
no shorter gap keeps the next offset = 2 mod 4) holds a canary bit pattern that must survive every
step: a store past a tensor would land on its bucket neighbour."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3), (40,), (257, 260), (1, 96), (96, 1)]
NUMEL = [torch.Size(s).numel() for s in SHAPES]
STEPS = 4
CANARY = 0x7A5B  # a bf16 bit pattern no average of these gradients rounds to in every element
CASES = [(rank, iters) for rank in (1, 2, 4) for iters in (1, 2, 3)]
PLACEMENTS = ("separate", "odd", "mod4")


def _mcr(rank: int, iters: int) -> float:
    # numel / (0.5 I r sum(shape)): (40,) is 2 / (I r), (1, 96) and (96, 1) are 1.979 / I
    return (1.99 if rank == 1 else 1.5) / iters


def _fresh(t: int):
    """Seeded bf16 gradients of step t whose scale grows each step (non-trivial residuals); a few
    -0.0 among them."""
    gen = torch.Generator().manual_seed(1000 + t)
    out = []
    for s in SHAPES:
        g = (torch.randn(s, generator=gen) * float(2 ** t)).to(BF16)
        g.view(-1)[::7] = -0.0
        out.append(g)
    return out


def _layout(placement: str):
    """Element offsets of the views in the bucket-like buffer, and its length."""
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
    """One destination set. `flat` (placements b, c): the bucket-like buffer, canary everywhere."""

    def __init__(self, placement: str, dev, fill_bits: int = CANARY):
        self.flat, self.offs = None, None
        if placement == "separate":
            self.views = [torch.empty(s, dtype=BF16, device=dev) for s in SHAPES]
            for v in self.views:
                v.view(torch.int16).fill_(fill_bits)
                assert v.data_ptr() % 16 == 0
            return
        self.offs, total = _layout(placement)
        self.flat = torch.empty(total, dtype=BF16, device=dev)
        self.flat.view(torch.int16).fill_(fill_bits)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[o:o + n].view(s) for o, n, s in zip(self.offs, NUMEL, SHAPES)]
        for v in self.views:
            if placement == "odd":
                assert v.data_ptr() % 4 == 2
            else:
                assert v.data_ptr() % 8 == 4
        self.outside = torch.ones(total, dtype=torch.bool, device=dev)
        for o, n in zip(self.offs, NUMEL):
            self.outside[o:o + n] = False
        assert bool(self.outside[:8].all()) and bool(self.outside[-8:].all())

    def canary_intact(self) -> bool:
        if self.flat is None:
            return True
        return bool((self.flat.view(torch.int16)[self.outside] == CANARY).all())


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


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
        """An fp32 residual (flat + views) and the PowerSGD over its views, on a fresh communicator."""
        from powersgd_amd import Config, PowerSGD

        residual = torch.zeros(sum(NUMEL), dtype=torch.float32, device=self.dev)
        views, off = [], 0
        for s, n in zip(SHAPES, NUMEL):
            views.append(residual[off:off + n].view(s))
            off += n
        inner = PowerSGD(views, Config(rank, _mcr(rank, iters), iters, 0))
        inner._powersgd._comm = self.comm()
        mask = inner.is_compressed_mask
        assert any(mask) and not all(mask), mask
        return residual, views, inner

    def _record(self, inner, residual, calls, final, dst):
        torch.cuda.synchronize()
        codec = inner._powersgd
        return {"calls": calls, "final": final, "dst": [_bits(d).cpu() for d in dst],
                "residual": _bits(residual).cpu(), "ps": _bits(codec._ps_buffer).cpu(),
                "qs": _bits(codec._qs_buffer).cpu()}

    def reference(self, rank, iters, steps=STEPS):
        """The defining sequence: residual += float(g) (what the hook's per-bucket ADD leaves),
        psgd_aggregate_comm on the residual, then the run-table GATHER (k_runs_mix) of the fp32
        averages into a dense bf16 buffer."""
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
        for t in range(steps):
            for v, g in zip(views, _fresh(t)):
                v.add_(g.to(self.dev).float())
            codec = inner._powersgd
            final = codec._plan.fused_final(codec.step_counter, False)
            n0 = self.stub.psgd_stub_calls()
            avg = inner.aggregate(views)
            _psgd_host.fill_list(avg, ctypes.addressof(out_ptrs), _lib.PSGD_F32, 0)
            bucket = torch.empty(sum(NUMEL), dtype=BF16, device=self.dev)
            bucket.view(torch.int16).fill_(CANARY)
            gather.gather(bucket.data_ptr(), ctypes.addressof(out_ptrs), self.stream)
            dst = [bucket[o:o + k] for o, k in zip(offs, NUMEL)]
            rec.append(self._record(inner, residual, self.stub.psgd_stub_calls() - n0, final, dst))
        inner.close()
        return rec

    def fused(self, rank, iters, placement, steps=STEPS, fill_bits=CANARY):
        """The direct call with PowerSGD.aggregate's bookkeeping (both step counters, the split by
        the compression mask), as the DDP hook makes it."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        residual, views, inner = self.codec(rank, iters)
        codec = inner._powersgd
        assert codec._plan.mixed_folds_dst(0, self.world) == 1 and codec._plan.mixed_folds_dst(1, self.world) == 1
        dst = _Dst(placement, self.dev, fill_bits)
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, _lib.PSGD_BF16, 0)
        rec = []
        for t in range(steps):
            for v, g in zip(views, _fresh(t)):
                v.add_(g.to(self.dev).float())
            final = codec._plan.fused_final(codec.step_counter, False)
            n0 = self.stub.psgd_stub_calls()
            table.fill(dst.views)
            inner.step_counter += 1
            inner._table.fill(views)
            codec._plan.aggregate_mixed_comm_dst(inner._table.comp_addr(), table.comp_addr(), codec.step_counter,
                                                 codec._comm, self.stream, flat=inner._unc.plan,
                                                 unc_residual=inner._table.unc_addr(), unc_dst_bf16=table.unc_addr())
            codec.step_counter += 1
            r = self._record(inner, residual, self.stub.psgd_stub_calls() - n0, final, [d.reshape(-1) for d in dst.views])
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


# ------------------------------------------------------------------ test 1
def _bitwise(_, init, world):
    ch = _Child(init, world)
    finals = set()
    try:
        for rank, iters in CASES:
            ref = ch.reference(rank, iters)  # computed once per case, shared by the placements, never modified
            assert [r["calls"] for r in ref] == [iters + 1] * STEPS, (world, rank, iters)
            assert any(bool(r["residual"].any()) for r in ref)  # the residuals are non-trivial
            for placement in PLACEMENTS:
                ctx = (world, rank, iters, placement)
                one = ch.fused(rank, iters, placement)
                _same(one, ref, ctx)
                assert all(r["canary"] for r in one), (ctx, [r["canary"] for r in one])
                # one collective per power iteration, the flat tail grouped with the last one
                assert [r["calls"] for r in one] == [iters + 1] * STEPS, (ctx, [r["calls"] for r in one])
                if placement == "odd":  # (the run-to-run check needs no second placement)
                    two = ch.fused(rank, iters, placement)
                    _same(two, one, (ctx, "second fused run"))
                finals |= {(rank, r["final"]) for r in one}
        # both final passes of the communicator sequence were reached: the apply pass (every rank
        # bucket) and the output pass after a fused k_final_odd (rank buckets 1 and 2)
        assert {(1, 0), (2, 0), (4, 0), (1, 1), (2, 1)} <= finals, finals
    finally:
        ch.close()


@pytest.mark.parametrize("world", [3, 4, 1])
def test_direct_call_equals_reference_sequence_bitwise(world, tmp_path):
    """Test 1: rank buckets 1 / 2 / 4 x 1-3 iterations x three placements x four steps, at W = 3,
    W = 4 and on a 1-rank communicator."""
    torch.multiprocessing.spawn(_bitwise, args=(_init(tmp_path), world), nprocs=1, join=True)


# ------------------------------------------------------------------ test 3
def _zero_negatives(_, init):
    ch = _Child(init, 3)
    try:
        for rank, iters in ((2, 2), (1, 1)):  # apply and low-rank final passes over two steps
            ref = ch.reference(rank, iters, steps=2)
            for placement in ("separate", "odd"):
                got = ch.fused(rank, iters, placement, steps=2, fill_bits=-0x8000)  # every element -0.0
                for t in range(2):
                    for i, (p, q) in enumerate(zip(got[t]["dst"], ref[t]["dst"])):
                        assert torch.equal(p, q), (rank, iters, placement, t, i)
    finally:
        ch.close()


def test_destinations_are_written_not_accumulated(tmp_path):
    """Test 3: destinations that hold -0.0 everywhere beforehand end with the reference's bits."""
    torch.multiprocessing.spawn(_zero_negatives, args=(_init(tmp_path),), nprocs=1, join=True)


# ------------------------------------------------------------------ test 2
def _refusals(_, init):
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    ch = _Child(init, 4)
    try:
        dev = ch.dev
        shapes = [(300, 520), (130, 67)]

        def state(codec):
            gen = torch.Generator().manual_seed(5)
            resid = [torch.randn(s, generator=gen).to(dev) for s in shapes]
            dst = [torch.full(s, 3.0, dtype=BF16, device=dev) for s in shapes]
            return resid, dst, resid + dst + [codec._ps_buffer, codec._qs_buffer]

        def unchanged(live, keep, n0, ctx):
            torch.cuda.synchronize()
            for a, b in zip(live, keep):
                assert torch.equal(_bits(a) if a.dtype == BF16 else a, _bits(b) if b.dtype == BF16 else b), ctx
            assert ch.stub.psgd_stub_calls() == n0, ctx

        def call(codec, resid, dst, comm):
            rp = _lib.ptr_array([r.data_ptr() for r in resid])
            dp = _lib.ptr_array([d.data_ptr() for d in dst])
            codec._plan.aggregate_mixed_comm_dst(ctypes.addressof(rp), ctypes.addressof(dp), 0, comm, ch.stream)

        for what in ("rank8", "bf16", "wide"):
            rank = {"rank8": 8, "bf16": 2, "wide": 64}[what]
            dt = BF16 if what == "bf16" else torch.float32
            codec = BasicPowerSGD([torch.zeros(s, dtype=dt, device=dev) for s in shapes], BasicConfig(rank, 2))
            assert codec._plan.is_wide() == (what == "wide")
            for w in (1, 4):
                assert codec._plan.mixed_folds_dst(0, w) == 0 and codec._plan.mixed_folds_dst(1, w) == 0
            comm = ch.comm()
            resid, dst, live = state(codec)
            keep = [x.clone() for x in live]
            n0 = ch.stub.psgd_stub_calls()
            with pytest.raises(ValueError, match="psgd_aggregate_mixed"):
                call(codec, resid, dst, comm)
            unchanged(live, keep, n0, what)

        # a poisoned communicator (a psgd_aggregate_comm call that failed past its argument checks:
        # a null gradient pointer, refused before anything runs) is refused at entry
        codec = BasicPowerSGD([torch.zeros(s, device=dev) for s in shapes], BasicConfig(2, 2))
        assert codec._plan.mixed_folds_dst(0, 4) == 1
        comm = ch.comm()
        resid, dst, live = state(codec)
        f32_out = torch.zeros(sum(torch.Size(s).numel() for s in shapes), device=dev)
        bad = _lib.ptr_array([0] * len(shapes))
        with pytest.raises(ValueError, match="null gradient pointer"):
            codec._plan.aggregate_comm(ctypes.addressof(bad), f32_out.data_ptr(), 0, None, None, 0, comm, ch.stream)
        keep = [x.clone() for x in live]
        n0 = ch.stub.psgd_stub_calls()
        with pytest.raises(RuntimeError, match="communicator unusable"):
            call(codec, resid, dst, comm)
        unchanged(live, keep, n0, "poisoned")
    finally:
        ch.close()


def test_refusals_touch_nothing(tmp_path):
    """Test 2: rank bucket 8, a bf16 plan and a wide plan are refused with PSGD_ERR_VALUE, a
    poisoned communicator at entry; destinations, residual, P/Q and the collective count stay."""
    torch.multiprocessing.spawn(_refusals, args=(_init(tmp_path),), nprocs=1, join=True)
