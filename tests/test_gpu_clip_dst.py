"""psgd_clip_dst (global-norm clipping after the direct-store completion: the averages scaled where
they lie, at per-tensor destinations) against the sequence it is defined as, on the same build and
the same communicator.

Flow X: psgd_aggregate_comm into the output slab and the dense uncompressed slab
(``PowerSGD.aggregate`` of the gradient views), then psgd_clip_outputs(form = 1) on the two slabs.
Flow Y: psgd_aggregate_comm_dst, then psgd_clip_dst on the same destination tables. psgd_clip_dst is
defined as copy-to-slabs, psgd_clip_outputs(form = 1), copy back, so there is no tolerance: after
every step the two result doubles are equal as raw bits, every destination is ``torch.equal`` on raw
bits to its slab view, and the residual and ``_ps_buffer`` / ``_qs_buffer`` are equal.

World size W runs on ONE GPU through the stand-in collective library (tests/stubs/rccl_stub.hip),
set up as tests/test_gpu_comm_dst.py does, at world 3 and on a 1-rank communicator. Shapes: those of
that file plus (41,): (256, 300) is longer than a scale item (8192 elements), (1,) is shorter than a
vector (uncompressed below rank bucket 4, a compressed 1 x 1 matrix from there on), (40,), (97,) and
(41,) never compress. All destinations live in one bucket-like buffer at element offsets = 1, 2 or 3
(mod 4), so every scale item has a head and a tail; every element outside the views holds a canary
that must survive every step.

Gradients grow 2 x per step. The threshold is the unclipped norm of step 1 (flow X at max_norm =
inf): step 0 lies below it (coef == 1.0, the destinations are the unclipped direct flow's bits),
steps 2 and 3 clip (coef < 1). Rank bucket 8 is not admitted for the destination form at I = 2 / 3
(tests/test_gpu_comm_dst.py pins that) and is left out."""
import ctypes
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
SHAPES = [(128, 64, 3, 3), (256, 300), (96, 200), (64, 100), (50, 150), (33, 65), (7, 5), (40,), (97,), (1,), (41,)]
NUMEL = [torch.Size(s).numel() for s in SHAPES]
STEPS = 4
CASES = [(1, 1), (1, 2), (2, 2), (4, 2), (4, 3), (16, 2), (32, 2)]  # (rank, iterations)
CANARY = 0x7FC12345  # a quiet NaN with a payload: no average is a NaN
PLACEMENTS = (1, 2, 3)  # element offset of every view modulo 4
ERR_LAYOUT, ERR_STATE = 4, 6  # psgd_status (include/psgd.h)


def _rate(shape, rank, iters):
    sh = list(shape)
    return torch.Size(sh).numel() / (0.5 * iters * min(rank, min(sh)) * sum(sh))


def _mcr(rank, iters):
    # 0.99 x the smallest rate of a 2-D shape: every 2-D shape compresses, (40,), (41,), (97,) never do
    return 0.99 * min(_rate(s, rank, iters) for s in SHAPES if len(s) > 1)


def _fresh(t, poison=False):
    """Seeded gradients of step t whose scale grows each step; a few -0.0. `poison`: one +inf element
    in the uncompressed (97,) tensor."""
    gen = torch.Generator().manual_seed(6000 + t)
    out = []
    for s in SHAPES:
        g = torch.randn(s, generator=gen) * float(2 ** t)
        g.view(-1)[::7] = -0.0
        out.append(g)
    if poison:
        out[8][5] = math.inf
    return out


def _layout(want):
    off, offs = 8, []
    for n in NUMEL:
        off += next(g for g in (1, 2, 3, 4) if (off + g) % 4 == want)
        offs.append(off)
        off += n
    return offs, off + 8


class _Dst:
    """One destination set: the bucket-like buffer, canary everywhere outside the views."""

    def __init__(self, want, dev):
        self.offs, total = _layout(want)
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat.view(torch.int32).fill_(CANARY)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[o:o + n].view(s) for o, n, s in zip(self.offs, NUMEL, SHAPES)]
        assert all(v.data_ptr() % 16 == 4 * want for v in self.views)
        self.outside = torch.ones(total, dtype=torch.bool, device=dev)
        for o, n in zip(self.offs, NUMEL):
            self.outside[o:o + n] = False
        assert all(bool(self.outside[o - 1]) and bool(self.outside[o + n]) for o, n in zip(self.offs, NUMEL))

    def canary_intact(self):
        return bool((self.flat.view(torch.int32)[self.outside] == CANARY).all())


def _bits(x):
    return x.contiguous().view(torch.int32)


class _Child:
    def __init__(self, init, world):
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
        self.world = world
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def codec(self, rank, iters):
        from powersgd_amd import Config, PowerSGD, _lib

        grads = torch.zeros(sum(NUMEL), dtype=torch.float32, device=self.dev)
        views, off = [], 0
        for s, n in zip(SHAPES, NUMEL):
            views.append(grads[off:off + n].view(s))
            off += n
        inner = PowerSGD(views, Config(rank, _mcr(rank, iters), iters, 0))
        inner._powersgd._comm = _lib.Comm(self.world, 0, _lib.comm_unique_id(), 0)
        mask = inner.is_compressed_mask
        assert all(mask[:7]) and not mask[7] and not mask[8] and not mask[10], (rank, iters, mask)
        assert inner._powersgd._plan.clip_dst_ok() == 1, (rank, iters)
        return grads, views, inner

    def _record(self, inner, grads, res, dst):
        torch.cuda.synchronize()
        codec = inner._powersgd
        out = {"dst": [_bits(d).cpu() for d in dst], "residual": _bits(grads).cpu(),
               "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu()}
        if res is not None:
            out["res_bits"] = res.view(torch.int64).cpu()
            out["norm"], out["coef"] = (float(x) for x in res.cpu())
        return out

    def flow_x(self, rank, iters, max_norm, steps=STEPS, poison=False):
        """psgd_aggregate_comm into the slabs, then psgd_clip_outputs(form = 1) on them."""
        grads, views, inner = self.codec(rank, iters)
        codec, u = inner._powersgd, inner._unc
        res = torch.zeros(2, dtype=torch.float64, device=self.dev)
        rec = []
        for t in range(steps):
            for v, g in zip(views, _fresh(t, poison)):
                v.add_(g.to(self.dev))
            avg = inner.aggregate(views)
            # the slabs are allocation bases, as the definition's
            assert codec._slab.data_ptr() % 256 == 0 and u.slab.data_ptr() % 256 == 0
            codec._plan.clip_outputs(codec.step_counter - 1, self.world, codec._slab.data_ptr(), u.slab.data_ptr(),
                                     u.numel, max_norm, res.data_ptr(), self.stream, form=codec._plan.NORM_FACTORS)
            rec.append(self._record(inner, grads, res, [a.reshape(-1) for a in avg]))
        inner.close()
        return rec

    def flow_y(self, rank, iters, max_norm, want, steps=STEPS, poison=False):
        """psgd_aggregate_comm_dst, then psgd_clip_dst (`max_norm` None: the unclipped direct flow)."""
        from powersgd_amd import _lib
        from powersgd_amd.powersgd import _psgd_host

        grads, views, inner = self.codec(rank, iters)
        codec = inner._powersgd
        assert codec._plan.dst_ok(0, self.world) == 1 and codec._plan.dst_ok(1, self.world) == 1, (rank, iters)
        dst = _Dst(want, self.dev)
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, _lib.PSGD_F32, 0)
        res = torch.zeros(2, dtype=torch.float64, device=self.dev) if max_norm is not None else None
        rec = []
        for t in range(steps):
            for v, g in zip(views, _fresh(t, poison)):
                v.add_(g.to(self.dev))
            table.fill(dst.views)
            inner.step_counter += 1
            inner._table.fill(views)
            kw = dict(flat=inner._unc.plan, unc_dst=table.unc_addr())
            codec._plan.aggregate_comm_dst(inner._table.comp_addr(), table.comp_addr(), codec.step_counter, codec._comm,
                                           self.stream, unc=inner._table.unc_addr(), **kw)
            if max_norm is not None:
                codec._plan.clip_dst(codec.step_counter, self.world, table.comp_addr(), max_norm, res.data_ptr(),
                                     self.stream, **kw)
            codec.step_counter += 1
            r = self._record(inner, grads, res, [d.reshape(-1) for d in dst.views])
            r["canary"] = dst.canary_intact()
            rec.append(r)
        inner.close()
        return rec

    def close(self):
        torch.distributed.destroy_process_group()


def _same(a, b, ctx, results=True):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        if results:
            assert torch.equal(x["res_bits"], y["res_bits"]), (ctx, t, "norm, coef", x["norm"], y["norm"], x["coef"], y["coef"])
        for i, (p, q) in enumerate(zip(x["dst"], y["dst"])):
            assert torch.equal(p, q), (ctx, t, i, "destination")
        for k in ("residual", "ps", "qs"):
            assert torch.equal(x[k], y[k]), (ctx, t, k)


def _init(tmp_path):
    return f"file://{tmp_path}/store"


# ------------------------------------------------------------------ test 1
def _bitwise(_, init, world):
    ch = _Child(init, world)
    try:
        for n, (rank, iters) in enumerate(CASES):
            x_inf = ch.flow_x(rank, iters, math.inf)  # the unclipped norms (and averages) of every step
            assert all(r["coef"] == 1.0 and math.isfinite(r["norm"]) and r["norm"] > 0 for r in x_inf), (world, rank, iters)
            thr = x_inf[1]["norm"]
            x = ch.flow_x(rank, iters, thr)  # once per case, shared by the placements, never modified
            assert [r["norm"] for r in x] == [r["norm"] for r in x_inf]  # clipping never feeds back
            assert x[0]["coef"] == 1.0 and x[2]["coef"] < 1.0 and x[3]["coef"] < 1.0, (world, rank, iters, x)
            assert any(bool(r["residual"].any()) for r in x)
            # max_norm = inf through the destination form: the norm, and nothing scaled
            want = PLACEMENTS[n % len(PLACEMENTS)]
            y_inf = ch.flow_y(rank, iters, math.inf, want)
            y_raw = ch.flow_y(rank, iters, None, want)  # the unclipped direct flow
            _same(y_inf, x_inf, (world, rank, iters, want, "inf"))
            _same(y_inf, y_raw, (world, rank, iters, want, "inf scales nothing"), results=False)
            for want in PLACEMENTS:
                ctx = (world, rank, iters, want)
                y = ch.flow_y(rank, iters, thr, want)
                _same(y, x, ctx)
                assert all(r["canary"] for r in y), (ctx, [r["canary"] for r in y])
                assert y[0]["coef"] == 1.0 and y[2]["coef"] < 1.0 and y[3]["coef"] < 1.0, ctx
                # step 0 is below the threshold: the unclipped direct flow's bits
                for i, (p, q) in enumerate(zip(y[0]["dst"], y_raw[0]["dst"])):
                    assert torch.equal(p, q), (ctx, i, "unclipped step")
                # ... and a clipping step changed them
                assert any(not torch.equal(p, q) for p, q in zip(y[3]["dst"], y_raw[3]["dst"])), ctx
    finally:
        ch.close()


@pytest.mark.parametrize("world", [3, 1])
def test_clip_dst_equals_defining_sequence_bitwise(world, tmp_path):
    """Seven (rank, iterations) cases x three placements x four steps, at W = 3 and on a 1-rank
    communicator."""
    torch.multiprocessing.spawn(_bitwise, args=(_init(tmp_path), world), nprocs=1, join=True)


# ------------------------------------------------------------------ test 2
def _nonfinite(_, init):
    ch = _Child(init, 3)
    try:
        for rank, iters, want in ((4, 2, 1), (1, 2, 3)):
            x = ch.flow_x(rank, iters, 1.0, steps=1, poison=True)
            y = ch.flow_y(rank, iters, 1.0, want, steps=1, poison=True)
            raw = ch.flow_y(rank, iters, None, want, steps=1, poison=True)
            assert math.isinf(y[0]["norm"]) and math.isnan(y[0]["coef"]), (rank, iters, y[0]["norm"], y[0]["coef"])
            _same(y, x, (rank, iters, "inf gradient"))
            _same(y, raw, (rank, iters, "inf gradient: untouched"), results=False)
            assert y[0]["canary"]
    finally:
        ch.close()


def test_nonfinite_norm_gives_nan_coef_and_scales_nothing(tmp_path):
    """One +inf gradient element: coef is NaN and the destinations are the unclipped flow's."""
    torch.multiprocessing.spawn(_nonfinite, args=(_init(tmp_path),), nprocs=1, join=True)


# ------------------------------------------------------------------ test 3
def _refusals(_, init):
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import _psgd_host

    ch = _Child(init, 3)
    try:
        L = _lib.lib()
        grads, views, inner = ch.codec(2, 2)
        codec, plan = inner._powersgd, inner._powersgd._plan
        dst = _Dst(1, ch.dev)
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, _lib.PSGD_F32, 0)
        table.fill(dst.views)
        res = torch.full((2,), -7.0, dtype=torch.float64, device=ch.dev)
        flat = inner._unc.plan
        live = [grads, dst.flat, res, codec._ps_buffer, codec._qs_buffer]

        def refused(code, msg, step, world, comp=None, unc=None, result=None):
            torch.cuda.synchronize()
            keep = [x.clone() for x in live]
            st = L.psgd_clip_dst(plan._h, step, world, comp or table.comp_addr(), flat._h, unc or table.unc_addr(), 1e-3,
                                 result or res.data_ptr(), ch.stream)
            torch.cuda.synchronize()
            assert st == code, (msg, st, L.psgd_last_error())
            assert msg.encode() in L.psgd_last_error(), (msg, L.psgd_last_error())
            for a, b in zip(live, keep):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), msg

        # no preceding step: the plan has recorded no output terms
        refused(ERR_STATE, "no record", 0, 3)
        for v, g in zip(views, _fresh(0)):
            v.add_(g.to(ch.dev))
        inner.step_counter += 1
        inner._table.fill(views)
        plan.aggregate_comm_dst(inner._table.comp_addr(), table.comp_addr(), 0, codec._comm, ch.stream, flat=flat,
                                unc=inner._table.unc_addr(), unc_dst=table.unc_addr())
        # another step, another world size than the record's
        refused(ERR_STATE, "no record", 1, 3)
        refused(ERR_STATE, "no record", 0, 2)
        # a destination at an odd byte address (a compressed tensor's, an uncompressed one's), the result
        nc = sum(inner.is_compressed_mask)
        comp = _lib.ptr_array([v.data_ptr() for v, c in zip(dst.views, inner.is_compressed_mask) if c])
        comp[nc - 1] += 2
        refused(ERR_LAYOUT, "4-byte aligned", 0, 3, comp=ctypes.addressof(comp))
        unc = _lib.ptr_array([v.data_ptr() for v, c in zip(dst.views, inner.is_compressed_mask) if not c])
        unc[0] += 1
        refused(ERR_LAYOUT, "4-byte aligned", 0, 3, unc=ctypes.addressof(unc))
        refused(ERR_LAYOUT, "8-byte aligned", 0, 3, result=res.data_ptr() + 4)
        # the refusals left the record usable: the call itself clips (the threshold is tiny)
        plan.clip_dst(0, 3, table.comp_addr(), 1e-3, res.data_ptr(), ch.stream, flat=flat, unc_dst=table.unc_addr())
        torch.cuda.synchronize()
        assert 0.0 < float(res[1]) < 1.0 and float(res[0]) > 1e-3
        assert dst.canary_intact()
        # a flat tail the plan never staged: a fresh plan after a slab step holds a record, no staging
        grads2, views2, inner2 = ch.codec(2, 2)
        for v, g in zip(views2, _fresh(0)):
            v.add_(g.to(ch.dev))
        inner2.aggregate(views2)
        plan2 = inner2._powersgd._plan
        torch.cuda.synchronize()
        before = dst.flat.clone()
        st = L.psgd_clip_dst(plan2._h, 0, 3, table.comp_addr(), inner2._unc.plan._h, table.unc_addr(), 1e-3,
                             res.data_ptr(), ch.stream)
        torch.cuda.synchronize()
        assert st == ERR_STATE and b"not staged" in L.psgd_last_error(), (st, L.psgd_last_error())
        assert torch.equal(_bits(before), _bits(dst.flat))
        inner.close()
        inner2.close()
    finally:
        ch.close()


def test_refusals_touch_nothing(tmp_path):
    """No preceding step, a step / world size that does not match the record, a destination at an odd
    byte address, a misaligned result and an unstaged flat tail are refused with their codes before
    anything is launched: destinations, result, residual and P/Q stay."""
    torch.multiprocessing.spawn(_refusals, args=(_init(tmp_path),), nprocs=1, join=True)
