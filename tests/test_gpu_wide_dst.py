"""psgd_aggregate_comm_dst_wide / psgd_aggregate_mixed_comm_dst_wide (ranks 33-128; k_wide_apply_dst) against the
sequence they are defined as, on the same build and communicator: psgd_aggregate_comm into slabs, then a copy
(bf16 form: ``.bfloat16()``) of every average to its destination, on raw bits; W = 3 through the stand-in collective
library (tests/test_gpu_comm_dst.py). Shapes: tests/test_gpu_wide_mixed.py's (odd m; a two-matrix group; a capped rank;
two full column tiles with one row past a block) plus an odd flat tensor. Destinations are views of one sentinel-filled
buffer with a gap after each: "packed" keeps every view after the first one element past a multiple of four (element
stores), "aligned" puts every view on a multiple of eight elements (16-byte / 8-byte stores where m % 4 == 0)."""
import ctypes
import types

import pytest
import torch

from test_gpu_comm_dst import _Child, _init

pytestmark = pytest.mark.gpu
SHAPES = [(130, 321), (96, 260), (96, 260), (100, 13), (65, 512), (257, 260), (40,), (41,)]
NUMEL = [torch.Size(s).numel() for s in SHAPES]
STEPS = 3
SENTINEL = {torch.float32: (torch.int32, 0x7FC12345), torch.bfloat16: (torch.int16, 0x7FC1)}  # quiet NaNs


def _fresh(t):
    gen = torch.Generator().manual_seed(2000 + t)
    return [torch.randn(s, generator=gen) * float(2 ** t) for s in SHAPES]


def _bits(x):
    return x.contiguous().view(SENTINEL[x.dtype][0]).reshape(-1)


def _codec(dev, rank, iters, comm):
    from powersgd_amd import Config, PowerSGD

    grads = torch.zeros(sum(NUMEL), device=dev)
    views = [g.view(s) for g, s in zip(grads.split(NUMEL), SHAPES)]
    inner = PowerSGD(views, Config(rank, 1.4 / iters, iters, 0))  # every matrix compresses (test_gpu_wide_mixed._mcr)
    assert inner.is_compressed_mask == [len(s) > 1 for s in SHAPES] and inner._powersgd._plan.is_wide()
    inner._powersgd._comm = comm
    return grads, views, inner


def _dst(dev, dtype, placement):
    off, offs = 8, []
    for n in NUMEL:
        offs.append(off)
        off += n + 1
        off += (-off) % 8 if placement == "aligned" else (1 - off) % 4
    it, pattern = SENTINEL[dtype]
    flat = torch.empty(off + 8, dtype=dtype, device=dev)
    flat.view(it).fill_(pattern)
    gaps = torch.ones(off + 8, dtype=torch.bool, device=dev)
    for o, n in zip(offs, NUMEL):
        gaps[o:o + n] = False
    return [flat[o:o + n].view(s) for o, n, s in zip(offs, NUMEL, SHAPES)], flat.view(it), gaps


def _run(ch, rank, iters, comm, dtype=None, placement=None, steps=STEPS):
    # `steps` steps of the new entry (`dtype`: its destinations') or, dtype None, of psgd_aggregate_comm
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import _psgd_host

    grads, views, inner = _codec(ch.dev, rank, iters, comm)
    codec, plan, rec = inner._powersgd, inner._powersgd._plan, []
    if dtype is not None:
        dst, raw, gaps = _dst(ch.dev, dtype, placement)
        code = _lib.PSGD_F32 if dtype == torch.float32 else _lib.PSGD_BF16
        table = _psgd_host.PtrTable([list(s) for s in SHAPES], inner.is_compressed_mask, code, 0)
        query, call = ((plan.dst_wide_ok, plan.aggregate_comm_dst_wide) if dtype == torch.float32
                       else (plan.mixed_dst_wide_ok, plan.aggregate_mixed_comm_dst_wide))
        assert query(0, ch.world) == 1 and query(1, ch.world) == 1, (rank, iters, ch.world, dtype)
        assert plan.dst_ok(0, ch.world) == 0 and plan.mixed_folds_dst(0, ch.world) == 0  # the narrow ones still refuse
    for t in range(steps):
        for v, g in zip(views, _fresh(t)):
            v.add_(g.to(ch.dev))
        n0 = ch.stub.psgd_stub_calls() if ch.stub else 0
        if dtype is None:
            out = [a.clone() for a in inner.aggregate(views)]
        else:
            table.fill(dst)
            inner._table.fill(views)
            names = ("unc", "unc_dst") if dtype == torch.float32 else ("unc_residual", "unc_dst_bf16")
            call(inner._table.comp_addr(), table.comp_addr(), codec.step_counter, comm, ch.stream,
                 flat=inner._unc.plan, **dict(zip(names, (inner._table.unc_addr(), table.unc_addr()))))
            codec.step_counter += 1
            out = dst
        torch.cuda.synchronize()
        rec.append({"out": [o.cpu() for o in out], "residual": _bits(grads).cpu(), "ps": _bits(codec._ps_buffer).cpu(),
                    "qs": _bits(codec._qs_buffer).cpu(), "calls": (ch.stub.psgd_stub_calls() if ch.stub else 0) - n0,
                    "gaps": dtype is None or bool((raw[gaps] == SENTINEL[dtype][1]).all())})
    if dtype is not None:  # the store widths this placement reaches: m % 4 == 0 and a 4-element aligned view
        rec[0]["vec"] = {s[1] % 4 == 0 and d.data_ptr() % (4 * d.element_size()) == 0 for s, d in zip(SHAPES, dst) if len(s) > 1}
    inner.close()
    return rec


def _entry(_, init, world, rank):
    ch = _Child(init, world)
    try:
        for iters in (1, 2):
            ref = _run(ch, rank, iters, ch.comm())  # once per case, shared by the forms and placements
            assert [r["calls"] for r in ref] == [iters + 1] * STEPS and any(bool(r["residual"].any()) for r in ref)
            for dtype in (torch.float32, torch.bfloat16):
                vec = []
                for placement in ("packed", "aligned"):
                    one = _run(ch, rank, iters, ch.comm(), dtype, placement)
                    vec.append(one[0]["vec"])
                    for t, (x, y) in enumerate(zip(one, ref)):
                        ctx = (world, rank, iters, dtype, placement, t)
                        for i, (a, b) in enumerate(zip(x["out"], y["out"])):
                            assert torch.equal(_bits(a), _bits(b.to(dtype))), (ctx, SHAPES[i], "destination")
                        for k in ("residual", "ps", "qs", "calls"):
                            assert torch.equal(torch.as_tensor(x[k]), torch.as_tensor(y[k])), (ctx, k)
                        assert x["gaps"], (ctx, "a gap lost its sentinel")
                assert vec == [{False}, {False, True}]  # from the pointers: element stores only; both widths
    finally:
        ch.close()


@pytest.mark.parametrize("rank", [33, 64, 100, 128])  # r % 4 != 0 at bucket 64, full 64, r < R at bucket 128, full 128
@pytest.mark.parametrize("world", [3, 1])
def test_wide_dst_entries_equal_their_definition_bitwise(world, rank, tmp_path):
    """Both entries, I = 1 and 2, both placements, three steps; every gap keeps its sentinel."""
    torch.multiprocessing.spawn(_entry, args=(_init(tmp_path), world, rank), nprocs=1, join=True)


def test_step0_against_float64():
    """Rank 64, I = 2, step 0, a null communicator, the bf16 form, restated in float64 from the codec's initial P / Q
    with tests/test_gpu_wide_mixed.py's bounds: the residual within 1e-5 of the input's norm, each bf16 average within
    2^-8 |ref| + 1e-5 max|input|. Guards against both sides of the bitwise test sharing a mistake."""
    dev = torch.device("cuda:0")  # world size 1 with a null communicator: no process group, no stub
    ch = types.SimpleNamespace(dev=dev, world=1, stub=None, stream=torch.cuda.current_stream(dev).cuda_stream)
    _, _, probe = _codec(ch.dev, 64, 2, None)
    p0, groups = probe._powersgd._ps_buffer.double().cpu(), probe._powersgd._plan.groups()
    probe.close()
    rec = _run(ch, 64, 2, None, torch.bfloat16, "packed", steps=1)[0]
    fresh, poff, off = _fresh(0), 0, [sum(NUMEL[:i]) for i in range(len(SHAPES))]
    for n, m, r, _ in groups:
        for i in [i for i, s in enumerate(SHAPES) if s == (n, m)]:
            G, P0 = fresh[i].double(), torch.linalg.qr(p0[poff:poff + n * r].view(n, r)).Q
            poff, Q0 = poff + n * r, G.t() @ P0
            Q1 = torch.linalg.qr(Q0).Q
            ref = P0 @ Q0.t() + ((G - P0 @ Q0.t()) @ Q1) @ Q1.t()
            res = rec["residual"][off[i]:off[i] + NUMEL[i]].view(torch.float32).view(n, m).double()
            res_err = float((res - (G - ref)).norm() / G.norm())
            out_err = float(((rec["out"][i].double() - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-5 * float(G.abs().max()))).max())
            print(f"{SHAPES[i]}: residual {res_err:.3e}, output error / bound {out_err:.3f}")
            assert res_err <= 1e-5 and out_err <= 1.0, (SHAPES[i], res_err, out_err)
    assert poff == p0.numel()
    for i in (6, 7):  # the flat tail at world size 1: the bf16 rounding of the input
        assert torch.equal(rec["out"][i], fresh[i].bfloat16())


def _refusals(_, init):
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    ch = _Child(init, 3)
    try:
        shapes, comm = [(96, 260), (100, 13)], ch.comm()
        for bf16 in (False, True):
            ddt = torch.bfloat16 if bf16 else torch.float32
            cases = [(torch.float32, 2, "ok", ValueError, "serves ranks 33-128"),
                     (torch.bfloat16, 64, "ok", ValueError if bf16 else RuntimeError, "takes an fp32 plan"),
                     (torch.float64, 2, "ok", ValueError if bf16 else RuntimeError, "takes an fp32 plan"),
                     (torch.float32, 64, "null", ValueError, "null argument"),
                     (torch.float32, 64, "null entry", ValueError, "null gradient pointer"),
                     (torch.float32, 64, "odd", RuntimeError, "-byte aligned")]
            for dt, rank, table, exc, msg in cases:
                torch.set_default_dtype(torch.float64 if dt == torch.float64 else torch.float32)  # P / Q follow it
                codec = BasicPowerSGD([torch.zeros(s, dtype=dt, device=ch.dev) for s in shapes], BasicConfig(rank, 2))
                torch.set_default_dtype(torch.float32)
                plan, gen = codec._plan, torch.Generator().manual_seed(5)
                assert rank == 64 and dt == torch.float32 or not any(q(0, w) for q in (plan.dst_wide_ok, plan.mixed_dst_wide_ok) for w in (1, 3))
                grads = [torch.randn(s, generator=gen).to(ch.dev).to(dt) for s in shapes]
                dst = [torch.full((torch.Size(s).numel() + 1,), 3.0, dtype=ddt, device=ch.dev) for s in shapes]
                ptrs = [dst[0].data_ptr(), {"null entry": 0, "odd": dst[1].data_ptr() + 1}.get(table, dst[1].data_ptr())]
                gp, dp = _lib.ptr_array([g.data_ptr() for g in grads]), _lib.ptr_array(ptrs)
                live = grads + dst + [codec._ps_buffer, codec._qs_buffer]
                keep, n0 = [x.clone() for x in live], ch.stub.psgd_stub_calls()
                call = plan.aggregate_mixed_comm_dst_wide if bf16 else plan.aggregate_comm_dst_wide
                with pytest.raises(exc, match=msg):
                    call(ctypes.addressof(gp), None if table == "null" else ctypes.addressof(dp), 0, comm, ch.stream)
                torch.cuda.synchronize()
                assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(live, keep)), (bf16, msg)
                assert ch.stub.psgd_stub_calls() == n0, (bf16, msg)
    finally:
        ch.close()


def test_refusals_touch_nothing(tmp_path):
    """Each refusal raises the documented code in both forms; gradients, destinations, P / Q and the call count stay."""
    torch.multiprocessing.spawn(_refusals, args=(_init(tmp_path),), nprocs=1, join=True)
