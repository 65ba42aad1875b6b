"""psgd_aggregate_mixed_comm_dst at rank buckets 16 and 32 (the DDP hook's one-call completion: the
matrix-core final pass of the communicator sequence stores each tensor's bf16 average at the
tensor's own destination) against the sequence it is defined as, on the same build and the same
communicator: psgd_aggregate_comm on the fp32 residual (``PowerSGD.aggregate`` of the residual
views) and the run-table GATHER of the fp32 averages into bf16.

Defined as that sequence, so there is no tolerance: ``torch.equal`` on raw bits, after every step,
of the destinations, the fp32 residual and the codec's ``_ps_buffer`` / ``_qs_buffer``.

World size 3 runs on ONE GPU through the stand-in collective library (tests/stubs/rccl_stub.hip),
set up as tests/test_gpu_mixed_comm_dst.py does; a 1-rank communicator runs the shared-term
instance. I = 2 takes the matrix-core tiles at both world sizes (4 and 2 staged panels); I = 3
sends every tile of W = 3 to the VALU fallback (6 panels > 4) and stays on the matrix cores at
W = 1. The shape set and its branch classes are those of tests/test_gpu_mixed_mfma.py.

The destinations are views of one bucket-like flat bf16 buffer in two placements:
  "even"  every view at an element offset that is a multiple of 4 (8-byte aligned): a row quad of
          a matrix-core tile is one 8-byte store;
  "odd"   every view at an odd element offset (2-byte aligned only): four 2-byte stores.
Both are asserted from the pointers. Every element outside the views (at least 8 before the first
view and after the last, 1-4 between neighbours) holds a canary bit pattern that must survive every
step: a store past a tensor would land on its bucket neighbour."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (24, 136), (130, 67), (64, 3, 3, 3), (40,), (257, 260), (1, 96), (96, 1)]
NUMEL = [torch.Size(s).numel() for s in SHAPES]
STEPS = 4
CANARY = 0x7A5B  # a bf16 bit pattern no average of these gradients rounds to in every element
CASES = [(rank, iters) for rank in (16, 32) for iters in (2, 3)]
PLACEMENTS = ("even", "odd")
MATRIX_CORE = (0, 1, 2)  # (300, 520) twice and (24, 136): m % 4 == 0 on 16-byte aligned residual views


def _mcr(iters: int) -> float:
    # numel / (0.5 I min(rank, min(shape)) sum(shape)): of the shapes with both matrix dimensions
    # above 1 the smallest is (24, 136) at rank 32, 1.7 / I; (40,) is 2 / (16 I) at most
    return 1.5 / iters


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
    want, mod = (1, 2) if placement == "odd" else (0, 4)
    off, offs = 8, []
    for n in NUMEL:
        off += next(g for g in (1, 2, 3, 4) if (off + g) % mod == want)
        offs.append(off)
        off += n
    return offs, off + 8


class _Dst:
    """One destination set: the bucket-like buffer, canary everywhere."""

    def __init__(self, placement: str, dev):
        self.offs, total = _layout(placement)
        self.flat = torch.empty(total, dtype=BF16, device=dev)
        self.flat.view(torch.int16).fill_(CANARY)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[o:o + n].view(s) for o, n, s in zip(self.offs, NUMEL, SHAPES)]
        for v in self.views:
            # the store form of the matrix-core tiles: 8 bytes / four 2-byte stores
            assert v.data_ptr() % 8 == 0 if placement == "even" else v.data_ptr() % 4 == 2
        self.outside = torch.ones(total, dtype=torch.bool, device=dev)
        for o, n in zip(self.offs, NUMEL):
            self.outside[o:o + n] = False
        assert bool(self.outside[:8].all()) and bool(self.outside[-8:].all())
        assert all(bool(self.outside[o - 1]) and bool(self.outside[o + n]) for o, n in zip(self.offs, NUMEL))

    def canary_intact(self) -> bool:
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
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def codec(self, rank, iters):
        """An fp32 residual (flat + views) and the PowerSGD over its views, on a fresh communicator."""
        from powersgd_amd import Config, PowerSGD, _lib

        residual = torch.zeros(sum(NUMEL), dtype=torch.float32, device=self.dev)
        views, off = [], 0
        for s, n in zip(SHAPES, NUMEL):
            views.append(residual[off:off + n].view(s))
            off += n
        inner = PowerSGD(views, Config(rank, _mcr(iters), iters, 0))
        inner._powersgd._comm = _lib.Comm(self.world, 0, _lib.comm_unique_id(), 0)
        mask = inner.is_compressed_mask
        for s, c in zip(SHAPES, mask):
            assert c or len(s) == 1 or 1 in s, (s, "both matrix dimensions above 1: compressed")
        assert not mask[SHAPES.index((40,))], mask
        for i in MATRIX_CORE:  # what sends a tile to the matrix cores follows the residual alone
            assert mask[i] and views[i].data_ptr() % 16 == 0 and views[i].shape[-1] % 4 == 0
        return residual, views, inner

    def _record(self, inner, residual, dst):
        torch.cuda.synchronize()
        codec = inner._powersgd
        return {"dst": [_bits(d).cpu() for d in dst], "residual": _bits(residual).cpu(),
                "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu()}

    def reference(self, rank, iters):
        """The defining sequence: residual += float(g) (what the hook's per-bucket ADD leaves),
        psgd_aggregate_comm on the residual, then the run-table GATHER of the fp32 averages into a
        dense bf16 buffer."""
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
            for v, g in zip(views, _fresh(t)):
                v.add_(g.to(self.dev).float())
            avg = inner.aggregate(views)
            _psgd_host.fill_list(avg, ctypes.addressof(out_ptrs), _lib.PSGD_F32, 0)
            bucket = torch.empty(sum(NUMEL), dtype=BF16, device=self.dev)
            bucket.view(torch.int16).fill_(CANARY)
            gather.gather(bucket.data_ptr(), ctypes.addressof(out_ptrs), self.stream)
            rec.append(self._record(inner, residual, [bucket[o:o + k] for o, k in zip(offs, NUMEL)]))
        inner.close()
        return rec

    def fused(self, rank, iters, placement):
        """The direct call with PowerSGD.aggregate's bookkeeping (both step counters, the split by
        the compression mask), as the DDP hook makes it."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        residual, views, inner = self.codec(rank, iters)
        codec = inner._powersgd
        assert codec._plan.mixed_folds_dst(0, self.world) == 1 and codec._plan.mixed_folds_dst(1, self.world) == 1
        dst = _Dst(placement, self.dev)
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, _lib.PSGD_BF16, 0)
        rec = []
        for t in range(STEPS):
            for v, g in zip(views, _fresh(t)):
                v.add_(g.to(self.dev).float())
            table.fill(dst.views)
            inner.step_counter += 1
            inner._table.fill(views)
            codec._plan.aggregate_mixed_comm_dst(inner._table.comp_addr(), table.comp_addr(), codec.step_counter,
                                                 codec._comm, self.stream, flat=inner._unc.plan,
                                                 unc_residual=inner._table.unc_addr(), unc_dst_bf16=table.unc_addr())
            codec.step_counter += 1
            r = self._record(inner, residual, [d.reshape(-1) for d in dst.views])
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


def _bitwise(_, init, world):
    ch = _Child(init, world)
    try:
        for rank, iters in CASES:
            ref = ch.reference(rank, iters)  # computed once per case, shared by the placements, never modified
            assert any(bool(r["residual"].any()) for r in ref)  # the residuals are non-trivial
            for placement in PLACEMENTS:
                ctx = (world, rank, iters, placement)
                one = ch.fused(rank, iters, placement)
                _same(one, ref, ctx)
                assert all(r["canary"] for r in one), (ctx, [r["canary"] for r in one])
                if placement == "odd":  # (the run-to-run check needs no second placement)
                    two = ch.fused(rank, iters, placement)
                    _same(two, one, (ctx, "second fused run"))
    finally:
        ch.close()


def _init(tmp_path):
    return f"file://{tmp_path}/store"


@pytest.mark.parametrize("world", [3, 1])
def test_direct_call_equals_reference_sequence_bitwise(world, tmp_path):
    """Rank buckets 16 / 32 x 2-3 iterations x two placements x four steps, at W = 3 and on a 1-rank
    communicator."""
    torch.multiprocessing.spawn(_bitwise, args=(_init(tmp_path), world), nprocs=1, join=True)
