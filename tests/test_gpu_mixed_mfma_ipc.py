"""The fused fp32-residual step over the IPC exchange (``PSGD_COMM=ipc``) at rank 16:
psgd_aggregate_mixed_ipc behind ``Fp32ResidualPowerSGD(..., fused=True)`` and
psgd_aggregate_mixed_ipc_dst (the DDP hook's form, called directly here) against the sequences they
are defined as on the same build: the run-table ADD, psgd_aggregate_ipc on the fp32 residual, the
run-table GATHER.

Defined as those sequences, so there is no tolerance: ``torch.equal`` on raw bits, after every
step, of the bf16 outputs, the fp32 residual and the codec's ``_ps_buffer`` / ``_qs_buffer``; the
consumed gradients must be +0.0 everywhere, and the ranks' outputs must agree bit for bit.

Two real processes on cuda:0 (``torch.multiprocessing.spawn``, a gloo group over a file store, as
tests/test_gpu_mixed_ipc.py), every rank with its OWN gradients (the seed includes the rank): the
local and the averaged factors differ. Rank 16, two iterations: two term sets x 2 terms, the
matrix-core tile's staging limit. The shape set and its branch classes are those of
tests/test_gpu_mixed_mfma.py; one spawn, both entries inside the workers."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (24, 136), (130, 67), (64, 3, 3, 3), (40,), (257, 260), (1, 96), (96, 1)]
NUMEL = [torch.Size(s).numel() for s in SHAPES]
STEPS = 3
WORLD = 2
RANK, ITERS = 16, 2
MCR = 1.5 / ITERS  # (24, 136) is 2.55 / I, the smallest with both dimensions above 1; (40,) is 0.125 / I
CANARY = 0x7A5B  # a bf16 bit pattern no average of these gradients rounds to in every element


def _fresh(t: int, rank_id: int):
    """Seeded bf16 gradients of step t on rank `rank_id` (every rank its own) whose scale grows each
    step (non-trivial residuals); a few -0.0 among them."""
    gen = torch.Generator().manual_seed(1000 + 17 * rank_id + t)
    out = []
    for s in SHAPES:
        g = (torch.randn(s, generator=gen) * float(2 ** t)).to(BF16)
        g.view(-1)[::7] = -0.0
        out.append(g)
    return out


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


def _check_mask(mask):
    for s, c in zip(SHAPES, mask):
        assert c or len(s) == 1 or 1 in s, (s, "both matrix dimensions above 1: compressed")
    assert not mask[SHAPES.index((40,))], mask


def _layout(odd: bool):
    """Element offsets of the destination views in the bucket-like buffer (odd, or a multiple of
    4: 8-byte aligned), and its length."""
    want, mod = (1, 2) if odd else (0, 4)
    off, offs = 8, []
    for n in NUMEL:
        off += next(g for g in (1, 2, 3, 4) if (off + g) % mod == want)
        offs.append(off)
        off += n
    return offs, off + 8


class _Rank:
    """One process of the group: PSGD_COMM=ipc, a gloo group over a file store, cuda:0."""

    def __init__(self, rank_id, initfile):
        os.environ["PSGD_COMM"] = "ipc"
        self.rank_id = rank_id
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=WORLD)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    # ---- psgd_aggregate_mixed_ipc behind the aggregator
    def flow(self, fused):
        from powersgd_amd import Config, Fp32ResidualPowerSGD

        agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=BF16, device=self.dev) for s in SHAPES],
                                   Config(RANK, MCR, ITERS, 0), fused=fused)
        _check_mask(agg.is_compressed_mask)
        codec = agg.inner._powersgd
        rec = []
        for t in range(STEPS):
            grads = [g.to(self.dev) for g in _fresh(t, self.rank_id)]
            folds = agg.fused_folds()
            out = agg.aggregate(grads)
            torch.cuda.synchronize()
            rec.append({
                "folds": folds,
                "out": [_bits(o).cpu() for o in out],
                "residual": _bits(agg.residual).cpu(),
                "ps": _bits(codec._ps_buffer).cpu(),
                "qs": _bits(codec._qs_buffer).cpu(),
                "grads_zero": all(not bool(_bits(g).any()) for g in grads),
            })
        assert codec._ipc_open
        assert not codec.ipc_status(), "a device-side exchange wait timed out"
        agg.close()
        return rec

    # ---- psgd_aggregate_mixed_ipc_dst, called directly
    def codec(self):
        """An fp32 residual (flat + views) and the PowerSGD over its views."""
        from powersgd_amd import Config, PowerSGD

        residual = torch.zeros(sum(NUMEL), dtype=torch.float32, device=self.dev)
        views, off = [], 0
        for s, n in zip(SHAPES, NUMEL):
            views.append(residual[off:off + n].view(s))
            off += n
        inner = PowerSGD(views, Config(RANK, MCR, ITERS, 0))
        _check_mask(inner.is_compressed_mask)
        return residual, views, inner

    def _record(self, inner, residual, dst):
        torch.cuda.synchronize()
        codec = inner._powersgd
        return {"out": [_bits(d).cpu() for d in dst], "residual": _bits(residual).cpu(),
                "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu(), "grads_zero": True}

    def _finish(self, inner):
        assert inner._powersgd._ipc_open and not inner._powersgd.ipc_status()
        inner.close()

    def dst_reference(self):
        """residual += float(g), psgd_aggregate_ipc on the residual into an fp32 slab
        (``PowerSGD.aggregate`` under PSGD_COMM=ipc), the run-table GATHER into a dense bf16 buffer."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        residual, views, inner = self.codec()
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
            gather.gather(bucket.data_ptr(), ctypes.addressof(out_ptrs), self.stream)
            rec.append(self._record(inner, residual, [bucket[o:o + k] for o, k in zip(offs, NUMEL)]))
        self._finish(inner)
        return rec

    def dst_fused(self, odd):
        """The direct call with PowerSGD.aggregate's bookkeeping, as the DDP hook makes it; the
        destinations are views of one bucket-like bf16 buffer, canary everywhere else."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        residual, views, inner = self.codec()
        codec = inner._powersgd
        assert codec._plan.mixed_folds_dst(0, WORLD) == 1 and codec._plan.mixed_folds_dst(1, WORLD) == 1
        offs, total = _layout(odd)
        flat = torch.empty(total, dtype=BF16, device=self.dev)
        flat.view(torch.int16).fill_(CANARY)
        dst = [flat[o:o + n].view(s) for o, n, s in zip(offs, NUMEL, SHAPES)]
        for v in dst:
            assert v.data_ptr() % 4 == 2 if odd else v.data_ptr() % 8 == 0
        outside = torch.ones(total, dtype=torch.bool, device=self.dev)
        for o, n in zip(offs, NUMEL):
            outside[o:o + n] = False
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, _lib.PSGD_BF16, 0)
        codec._ipc_setup(inner._unc.numel)
        rec = []
        for t in range(STEPS):
            for v, g in zip(views, _fresh(t, self.rank_id)):
                v.add_(g.to(self.dev).float())
            table.fill(dst)
            inner.step_counter += 1
            inner._table.fill(views)
            codec._plan.aggregate_mixed_ipc_dst(inner._table.comp_addr(), table.comp_addr(), codec.step_counter,
                                                self.stream, flat=inner._unc.plan,
                                                unc_residual=inner._table.unc_addr(), unc_dst_bf16=table.unc_addr())
            codec.step_counter += 1
            rec.append(self._record(inner, residual, [d.reshape(-1) for d in dst]))
            assert bool((flat.view(torch.int16)[outside] == CANARY).all()), (odd, t, "canary")
        self._finish(inner)
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


def _agree(rec, ctx):
    """The averages are the same on every rank; every rank keeps the error of ITS gradients."""
    mine = {"out": [r["out"] for r in rec], "residual": rec[-1]["residual"]}
    every = [None] * WORLD
    torch.distributed.all_gather_object(every, mine)
    for w, other in enumerate(every):
        for t in range(STEPS):
            for i, (p, q) in enumerate(zip(mine["out"][t], other["out"][t])):
                assert torch.equal(p, q), (ctx, w, t, i, "the averages are the same on every rank")
    assert not torch.equal(every[0]["residual"], every[1]["residual"]), ctx


def _worker(rank_id, initfile):
    me = _Rank(rank_id, initfile)
    try:
        ref = me.flow(False)  # the reference: computed once, never modified
        assert [r["folds"] for r in ref] == [(0, 0)] * STEPS  # fused=False never folds
        one = me.flow(True)
        print(rank_id, "folds", [r["folds"] for r in one], flush=True)
        _same(one, ref, (rank_id, "psgd_aggregate_mixed_ipc"))
        assert [r["folds"] for r in one] == [(0, 1)] * STEPS, [r["folds"] for r in one]
        assert any(bool(r["residual"].any()) for r in one)  # the residuals are non-trivial
        _agree(one, (rank_id, "psgd_aggregate_mixed_ipc"))

        dref = me.dst_reference()  # shared by the two placements, never modified
        for odd in (False, True):
            got = me.dst_fused(odd)
            _same(got, dref, (rank_id, "psgd_aggregate_mixed_ipc_dst", odd))
            _agree(got, (rank_id, "psgd_aggregate_mixed_ipc_dst", odd))
    finally:
        me.close()


def test_fused_ipc_forms_equal_their_sequences_bitwise(tmp_path):
    """Rank 16, I = 2, W = 2 (real processes, distinct gradients): psgd_aggregate_mixed_ipc and
    psgd_aggregate_mixed_ipc_dst (8-byte aligned and odd-offset destinations, canaries around them)
    against their three-stage IPC sequences; the ranks agree bit for bit."""
    torch.multiprocessing.spawn(_worker, args=(os.path.join(str(tmp_path), "init"),), nprocs=WORLD, join=True)
