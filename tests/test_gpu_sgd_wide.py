"""The fused SGD step at ranks 33-128 (include/psgd.h: psgd_aggregate_comm_sgd_wide; k_wide_apply_sgd,
psgd_wide_sgd.hip).

Test 1 has no tolerance: the entry is DEFINED as psgd_aggregate_comm on the same wide plan (fp32 slabs) followed by
psgd_sgd_update; the averages have k_wide_apply<float>'s bits by construction and sgd_update is one device function,
so raw bits are compared. test_gpu_comm_dst's shapes are the smallest that reach every path of a 64 x 256 tile at
these ranks (test_gpu_adam_wide.py lists them). Tests 2 and 3 use THE BOUND of test_gpu_sgd_step.py exactly as there."""
import ctypes

import pytest
import torch

from test_gpu_comm_dst import NUMEL, SHAPES, _bits, _Child, _Dst, _fresh, _init
from test_gpu_sgd_step import HYPER, _ref64

pytestmark = pytest.mark.gpu
STEPS = 3  # `first` taken once and not taken twice
PLACES = (("aligned", "aligned"), ("one_in", "one_in"), ("aligned", "one_in"))  # of p, buf; the last two: element form


def _run(ch, rank, iters, hp, fused, places=PLACES[0], comm=True):
    """STEPS steps of the wide entry (`fused`) or of its defining sequence (which also records its averages)."""
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import _psgd_host

    grads, views, inner = ch.codec(rank, iters)
    codec, plan = inner._powersgd, inner._powersgd._plan
    assert plan.is_wide()
    assert all(plan.sgd_wide_ok(par, ch.world, m) == 1 for par in (0, 1) for m in (False, True)), (rank, iters, ch.world)
    assert plan.sgd_ok(0, ch.world) == 0  # the narrow entry still refuses
    mom = hp[1] != 0
    P, B = _Dst(places[0], ch.dev), _Dst(places[1], ch.dev)
    gen = torch.Generator().manual_seed(77)
    for x in P.views:
        x.copy_(torch.randn(x.shape, generator=gen))
    for x in B.views:
        x.zero_()
    b0 = _bits(B.flat).clone()
    mask, n = inner.is_compressed_mask, len(SHAPES)
    tabs = [_psgd_host.PtrTable([list(s) for s in SHAPES], mask, _lib.PSGD_F32, 0) for _ in range(2)]
    order = [i for i, c in enumerate(mask) if c] + [i for i, c in enumerate(mask) if not c]
    # without momentum the buffer table is NULL, or (mixed placement) a placeholder that must stay untouched
    with_b = mom or places[0] != places[1]
    rec = [{"p": [_bits(x).cpu() for x in P.views], "buf": [_bits(x).cpu() for x in B.views]}]  # the initial state
    for t in range(STEPS):
        for v, g in zip(views, _fresh(t)):
            v.add_(g.to(ch.dev))
        hyper = _lib.sgd_hyper([hp + (t == 0,)] * n)
        n0, avg = ch.stub.psgd_stub_calls(), None
        if fused:
            inner._table.fill(views)
            for tab, d in zip(tabs, (P, B)):
                tab.fill(d.views)
            plan.aggregate_comm_sgd(inner._table.comp_addr(), tabs[0].comp_addr(), tabs[1].comp_addr() if with_b else None,
                                    hyper, codec.step_counter, codec._comm if comm else None, ch.stream,
                                    flat=inner._unc.plan, unc=inner._table.unc_addr(), unc_params=tabs[0].unc_addr(),
                                    unc_bufs=tabs[1].unc_addr() if with_b else None, wide=True)
            codec.step_counter += 1
        else:
            avg = inner.aggregate(views)  # psgd_aggregate_comm: the fp32 slab and the flat slab
            arr = [_lib.ptr_array([xs[i].data_ptr() for i in order]) for xs in (avg, P.views, B.views)]
            g_, p_, b_ = (ctypes.addressof(a) for a in arr)
            _lib.sgd_update(plan, g_, p_, b_ if mom else None, [NUMEL[i] for i in order], hyper, ch.stream)
        torch.cuda.synchronize()
        rec.append({"calls": ch.stub.psgd_stub_calls() - n0, "residual": _bits(grads).cpu(),
                    "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu(),
                    "canary": P.canary_intact() and B.canary_intact(), "avg": avg and [a.cpu() for a in avg],
                    "p": [_bits(x).cpu() for x in P.views], "buf": [_bits(x).cpu() for x in B.views]})
    assert mom or torch.equal(_bits(B.flat), b0), "buf is neither read nor written without momentum"
    inner.close()
    return rec


def _entry(_, init, world, rank):
    ch = _Child(init, world)
    try:
        for iters in (1, 2):
            for name in ("plain", "nesterov"):
                ref = _run(ch, rank, iters, HYPER[name], False)  # once per case, shared by the placements
                assert [r["calls"] for r in ref[1:]] == [iters + 1] * STEPS and any(bool(r["residual"].any()) for r in ref[1:])
                cases = [(pl, True) for pl in PLACES] + ([(PLACES[1], False)] if world == 1 else [])  # a null communicator
                for places, comm in cases:
                    one = _run(ch, rank, iters, HYPER[name], True, places, comm)
                    for t, (x, y) in enumerate(zip(one[1:], ref[1:])):
                        ctx = (world, rank, iters, name, places, comm, t)
                        for k in ("p", "buf"):
                            assert all(torch.equal(a, b) for a, b in zip(x[k], y[k])), (ctx, k)
                        for k in ("residual", "ps", "qs"):
                            assert torch.equal(x[k], y[k]), (ctx, k)
                        assert x["calls"] == (y["calls"] if comm else 0), (ctx, "collective count")
                        assert x["canary"], ctx
    finally:
        ch.close()


# r % 4 != 0 at bucket 64, full 64, r < R at bucket 128, full 128; two ranks (two term sets) once, at rank 64
@pytest.mark.parametrize("world,rank", [(1, 33), (1, 64), (1, 100), (1, 128), (2, 64)])
def test_wide_entry_equals_its_definition_bitwise(world, rank, tmp_path):
    """psgd_aggregate_comm_sgd_wide against psgd_aggregate_comm + psgd_sgd_update: raw bits of every p, buf, the
    residual, the P/Q state and the collective count after each of 3 steps, I = 1 and 2, without momentum and with
    momentum + weight decay + nesterov, three placements of p / buf, canaries intact; the query 1 at both parities."""
    torch.multiprocessing.spawn(_entry, args=(_init(tmp_path), world, rank), nprocs=1, join=True)


def _f64(_, init):
    ch = _Child(init, 1)
    try:
        f = lambda xs: [x.view(torch.float32) for x in xs]  # noqa: E731
        ref, one = (_run(ch, 64, 2, HYPER["mom_wd"], fused) for fused in (False, True))
        for t in range(STEPS):  # the two runs' states are bit for bit the same (test 1): ref[t] is the state before
            for i, (g, p0, b0, p1, b1) in enumerate(zip(ref[t + 1]["avg"], f(ref[t]["p"]), f(ref[t]["buf"]),
                                                        f(one[t + 1]["p"]), f(one[t + 1]["buf"]))):
                want_p, want_b, bound, bound_b = _ref64(HYPER["mom_wd"], t == 0, g, p0, b0)
                assert bool(((p1.double() - want_p).abs() <= bound).all()), (t, i, "p")
                assert bool(((b1.double() - want_b).abs() <= bound_b).all()), (t, i, "buf")
    finally:
        ch.close()


def test_wide_entry_against_float64(tmp_path):
    """Rank 64, I = 2, momentum + weight decay: p' and buf' within THE BOUND k 2^-24 S of the float64 formula
    evaluated on psgd_aggregate_comm's averages, from the same state, on the first step and on two later ones."""
    torch.multiprocessing.spawn(_f64, args=(_init(tmp_path),), nprocs=1, join=True)


def _refused(_, init):
    from powersgd_amd import Config, PowerSGD, _lib

    ch = _Child(init, 1)
    try:
        a = ctypes.addressof
        tab = lambda xs: _lib.ptr_array([x.data_ptr() for x in xs])  # noqa: E731
        hyper = _lib.sgd_hyper([HYPER["mom_wd"] + (True,)])
        cold = _lib.Plan([(128, 128)], 64, 1, _lib.PSGD_F32)  # never bound
        for rank, dtype, match in ((64, torch.float32, None), (32, torch.float32, "serves ranks 33-128"),
                                   (64, torch.bfloat16, "takes an fp32 plan")):
            g = [torch.ones(128, 128, dtype=dtype, device=ch.dev)]
            p, b = [torch.ones(128, 128, device=ch.dev)], [torch.ones(128, 128, device=ch.dev)]
            agg = PowerSGD(g, Config(rank, 0.5, 1, 0))  # owns the bound plan
            plan = agg._powersgd._plan
            gt, pt, bt, nul = tab(g), tab(p), tab(b), _lib.ptr_array([0])
            call = lambda pl, gg, pp, bb, hh: pl.aggregate_comm_sgd(gg, pp, bb, hh, 0, None, ch.stream, wide=True)  # noqa: E731
            if match:  # a narrow plan, a bf16 plan
                with pytest.raises((ValueError, RuntimeError), match=match):
                    call(plan, a(gt), a(pt), a(bt), hyper)
                assert plan.sgd_wide_ok(0, 1) == 0
                continue
            for args in ((None, a(pt), a(bt), hyper), (a(gt), None, a(bt), hyper), (a(gt), a(pt), a(bt), None)):
                with pytest.raises(ValueError, match="null argument"):
                    call(plan, *args)
            with pytest.raises(RuntimeError, match="not bound"):
                call(cold, a(gt), a(pt), a(bt), hyper)
            for bb in (None, a(nul)):  # no table, a null entry: momentum is 0.9
                with pytest.raises(ValueError, match="null momentum buffer"):
                    call(plan, a(gt), a(pt), bb, hyper)
            torch.cuda.synchronize()
            assert all(bool((x == 1).all()) for x in g + p + b)  # nothing ran
    finally:
        ch.close()


def test_wide_entry_refusals(tmp_path):
    torch.multiprocessing.spawn(_refused, args=(_init(tmp_path),), nprocs=1, join=True)


# ------------------------------------------------------------------ sgd_step at rank 64
MODEL = [(96, 260), (130, 321), (100, 13), (50,)]  # rates 0.88 / 1.09 / 1.44 at rank 64, I = 2; the bias stays dense
HP = HYPER["mom_wd"]


def _setup(**kw):
    from powersgd_amd import Config, PowerSGD

    gen = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to("cuda:0")) for s in MODEL]
    opt = torch.optim.SGD(params, lr=HP[0], momentum=HP[1], weight_decay=HP[3], foreach=False)
    agg = PowerSGD(params, Config(64, 0.5, 2, 1), **kw)
    assert agg._powersgd._plan.is_wide()
    return params, opt, agg


def _parity(_, initfile):
    from powersgd_amd import optimizer_step, sgd_step, sgd_step_applies

    torch.cuda.set_device(0)
    torch.distributed.init_process_group("nccl", init_method=f"file://{initfile}", rank=0, world_size=1,
                                         device_id=torch.device("cuda:0"))
    try:
        (pa, oa, ga), (pb, ob, gb), (pc, oc, gc) = _setup(), _setup(), _setup(max_grad_norm=1.0)
        seen = {}
        ob.register_step_pre_hook(lambda *_: seen.update(g=[p.grad.detach().clone() for p in pb]))
        for t in range(3):  # one warm-up step, then both parities
            before = [(y.data.clone(), ob.state[y]["momentum_buffer"].clone()) for y in pb] if t else None
            gen = torch.Generator().manual_seed(500 + t)
            for x, y, z in zip(pa, pb, pc):
                x.grad = torch.randn(x.shape, generator=gen).to(x.device) + (0 if x.grad is None else x.grad)
                y.grad, z.grad = x.grad.clone(), x.grad.clone()
            assert sgd_step_applies(oa, ga) == (t >= 1), t
            gc.step_counter = ga.step_counter
            assert not sgd_step_applies(oc, gc), "max_grad_norm keeps optimizer_step"
            sgd_step(oa, ga)
            optimizer_step(ob, gb)
            torch.cuda.synchronize()
            for i, (x, y) in enumerate(zip(pa, pb)):
                assert torch.equal(_bits(x.grad), _bits(y.grad)), (t, i, "residual")
                bx, by = oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"]
                if t:
                    _, _, bound, bound_b = _ref64(HP, False, seen["g"][i].cpu(), *(s.cpu() for s in before[i]))
                    assert bool(((x.data - y.data).cpu().double().abs() <= 2 * bound).all()), (t, i, "p")
                    assert bool(((bx - by).cpu().double().abs() <= 2 * bound_b).all()), (t, i, "buf")
                x.data.copy_(y.data)  # identical state before the next step: bounds do not compound
                bx.copy_(by)
    finally:
        torch.distributed.destroy_process_group()


def test_sgd_step_takes_the_wide_entry_at_rank_64(tmp_path):
    """sgd_step on a rank-64 plan in a one-rank process group: sgd_step_applies true on the compressing steps (false
    with max_grad_norm), the residual bitwise optimizer_step's, p and momentum_buffer within 2 x THE BOUND of
    optimizer_step + torch.optim.SGD from the same state."""
    torch.multiprocessing.spawn(_parity, args=(str(tmp_path / "init"),), nprocs=1, join=True)
