"""The fused Adam / AdamW steps at ranks 33-128 (include/psgd.h: psgd_aggregate_comm_adam_wide,
psgd_aggregate_mixed_comm_adam_wide; k_wide_apply_adam, psgd_wide_adam.hip).

Test 1 has no tolerance: the entries are DEFINED as psgd_aggregate_comm on the same wide plan (fp32 slabs) followed by
psgd_adam_update / psgd_adam_update_mp (for the master-weight form after the ADD of the bf16 gradients into the
residual); the averages have k_wide_apply<float>'s bits by construction and adam_update is one device function, so
raw bits are compared. test_gpu_comm_dst's shapes are the smallest that reach every path of a 64 x 256 tile at these
ranks: (256, 300) crosses a column tile, (128, 64, 3, 3) is three column tiles, (96, 200) and (50, 150) have rows
that do not fill a block, (33, 65) has m % 4 != 0 (element accesses, r capped at 33), (7, 5) has r = 5, and (40,),
(97,), (1,) are the flat tail. Test 2 uses THE BOUND of test_gpu_adam_step.py exactly as there."""
import ctypes

import pytest
import torch

from test_gpu_adam_master import W_CANARY, _b16, _W
from test_gpu_adam_step import HYPER, KEYS, _backward, _ref64, _within
from test_gpu_comm_dst import NUMEL, SHAPES, _bits, _Child, _Dst, _fresh, _init

pytestmark = pytest.mark.gpu
STEPS = 3
PLACES = (("aligned",) * 3, ("one_in",) * 3, ("aligned", "aligned", "one_in"))  # of p, m, v; the last: element form


def _run(ch, rank, iters, hp, mp, fused, places=PLACES[0], shift=0, comm=True):
    """STEPS steps of the wide entry (`fused`) or of its defining sequence; `mp`: the master-weight form."""
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import _psgd_host

    grads, views, inner = ch.codec(rank, iters)  # mp: the fp32 residual
    codec, plan = inner._powersgd, inner._powersgd._plan
    assert plan.is_wide()
    query = plan.mixed_adam_wide_ok if mp else plan.adam_wide_ok
    assert query(0, ch.world) == 1 and query(1, ch.world) == 1, (rank, iters, ch.world, mp)
    assert plan.adam_ok(0, ch.world) == 0 and plan.mixed_adam_ok(0, ch.world) == 0  # the narrow entries still refuse
    state = [_Dst(pl, ch.dev) for pl in places]  # p, m, v
    gen = torch.Generator().manual_seed(77)
    for x in state[0].views:
        x.copy_(torch.randn(x.shape, generator=gen))
    for d in state[1:]:
        for x in d.views:
            x.zero_()
    w = _W(shift, ch.dev)
    g16 = [torch.zeros(s, dtype=torch.bfloat16, device=ch.dev) for s in SHAPES]
    mask, n = inner.is_compressed_mask, len(SHAPES)
    f32 = [_psgd_host.PtrTable([list(s) for s in SHAPES], mask, _lib.PSGD_F32, 0) for _ in range(3)]
    b16 = [_psgd_host.PtrTable([list(s) for s in SHAPES], mask, _lib.PSGD_BF16, 0) for _ in range(2)]
    add = _lib.Runs([0] * n, list(range(n)), [0] * n, NUMEL, n, _lib.PSGD_F32, _lib.PSGD_BF16, source=list(range(n)), nsources=n)
    ws = torch.empty(add.workspace_bytes(), dtype=torch.uint8, device=ch.dev)
    add.bind(0, ws.data_ptr())
    order = [i for i, c in enumerate(mask) if c] + [i for i, c in enumerate(mask) if not c]
    rec = []
    for t in range(STEPS):
        for x, v, g in zip(g16, views, _fresh(t)):
            x.copy_(g.to(ch.dev)) if mp else v.add_(g.to(ch.dev))
        hyper = _lib.adam_hyper([hp + (float(t + 1),)] * n)
        n0 = ch.stub.psgd_stub_calls()
        hold = []  # the pointer arrays of this step's calls
        arr = lambda xs: hold.append(_lib.ptr_array([x.data_ptr() for x in xs])) or ctypes.addressof(hold[-1])  # noqa: E731
        if fused:
            inner._table.fill(views)
            for tab, d in zip(f32 + b16, state + [w]):
                tab.fill(d.views)
            b16[1].fill(g16)
            kw = dict(flat=inner._unc.plan, unc_ms=f32[1].unc_addr(), unc_vs=f32[2].unc_addr(), wide=True)
            tail = (hyper, codec.step_counter, codec._comm if comm else None, ch.stream)
            if mp:
                plan.aggregate_mixed_comm_adam(b16[1].comp_addr(), inner._table.comp_addr(), b16[0].comp_addr(),
                                               *(x.comp_addr() for x in f32), *tail, unc_bf16=b16[1].unc_addr(),
                                               unc_residual=inner._table.unc_addr(), unc_params_bf16=b16[0].unc_addr(),
                                               unc_masters=f32[0].unc_addr(), **kw)
            else:
                plan.aggregate_comm_adam(inner._table.comp_addr(), *(x.comp_addr() for x in f32), *tail,
                                         unc=inner._table.unc_addr(), unc_params=f32[0].unc_addr(), **kw)
            codec.step_counter += 1
        else:
            if mp:
                add.add_list(arr(g16), arr(views), True, ch.stream)
            avg = inner.aggregate(views)  # psgd_aggregate_comm: the fp32 slab and the flat slab
            lists = [[xs[i] for i in order] for xs in [avg] + [d.views for d in state]]
            if mp:
                _lib.adam_update_mp(plan, *(arr(xs) for xs in lists), arr([w.views[i] for i in order]),
                                    [NUMEL[i] for i in order], hyper, ch.stream)
            else:
                _lib.adam_update(plan, *(arr(xs) for xs in lists), [NUMEL[i] for i in order], hyper, ch.stream)
        torch.cuda.synchronize()
        rec.append({"calls": ch.stub.psgd_stub_calls() - n0, "residual": _bits(grads).cpu(),
                    "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu(),
                    "canary": all(d.canary_intact() for d in state + [w]),
                    "g16": [_b16(x).cpu() for x in g16], "w": [_b16(x).cpu() for x in w.views],
                    **{k: [_bits(x).cpu() for x in d.views] for k, d in zip("pmv", state)}})
    inner.close()
    return rec


def _entry(_, init, world, rank):
    ch = _Child(init, world)
    try:
        for iters in (1, 2):
            for name in ("adam_l2", "adamw"):
                for mp in (False, True):
                    ref = _run(ch, rank, iters, HYPER[name], mp, False)  # once per case, shared by the placements
                    assert [r["calls"] for r in ref] == [iters + 1] * STEPS and any(bool(r["residual"].any()) for r in ref)
                    cases = [(pl, sh, True) for pl, sh in zip(PLACES, (0, 1, 0) if mp else (0, 0, 0))]
                    cases += [(PLACES[1], 0, False)] if world == 1 else []  # a null communicator: no collective
                    for places, shift, comm in cases:
                        one = _run(ch, rank, iters, HYPER[name], mp, True, places, shift, comm)
                        for t, (x, y) in enumerate(zip(one, ref)):
                            ctx = (world, rank, iters, name, mp, places, shift, comm, t)
                            for k in ["p", "m", "v"] + (["w", "g16"] if mp else []):
                                assert all(torch.equal(a, b) for a, b in zip(x[k], y[k])), (ctx, k)
                            for k in ("residual", "ps", "qs"):
                                assert torch.equal(x[k], y[k]), (ctx, k)
                            assert x["calls"] == (y["calls"] if comm else 0), (ctx, "collective count")
                            assert x["canary"], ctx
                            assert not mp or not any(bool((a == W_CANARY).any()) for a in x["w"]), (ctx, "w never stored")
    finally:
        ch.close()


@pytest.mark.parametrize("rank", [33, 64, 100, 128])  # r % 4 != 0 at bucket 64, full 64, r < R at bucket 128, full 128
@pytest.mark.parametrize("world", [3, 1])
def test_wide_entries_equal_their_definition_bitwise(world, rank, tmp_path):
    """Both wide entries against psgd_aggregate_comm + psgd_adam_update[_mp]: raw bits of every p, m, v (w, and the
    zeroed bf16 gradients), the residual, the P/Q state and the collective count after each of 3 steps, I = 1 and 2,
    three placements of p / m / v, w aligned and one element in, canaries intact; both queries 1 at both parities."""
    torch.multiprocessing.spawn(_entry, args=(_init(tmp_path), world, rank), nprocs=1, join=True)


def _refused(_, init):
    from powersgd_amd import _lib

    ch = _Child(init, 3)
    try:
        grads, views, inner = ch.codec(32, 1)
        codec, plan = inner._powersgd, inner._powersgd._plan
        assert all(q(par, w) == 0 for q in (plan.adam_wide_ok, plan.mixed_adam_wide_ok) for par in (0, 1) for w in (1, 3))
        for v, g in zip(views, _fresh(0)):
            v.add_(g.to(ch.dev))
        state = [_Dst("aligned", ch.dev) for _ in range(3)]
        w = _W(0, ch.dev)
        g16 = [torch.ones(s, dtype=torch.bfloat16, device=ch.dev) for s in SHAPES]
        comp = [i for i, c in enumerate(inner.is_compressed_mask) if c]
        unc = [i for i, c in enumerate(inner.is_compressed_mask) if not c]
        tab = lambda xs, idx: _lib.ptr_array([xs[i].data_ptr() for i in idx])  # noqa: E731
        sets = [views] + [d.views for d in state] + [g16, w.views]
        ct, ut = [tab(xs, comp) for xs in sets], [tab(xs, unc) for xs in sets]
        c, u = [ctypes.addressof(x) for x in ct], [ctypes.addressof(x) for x in ut]
        live = [grads, codec._ps_buffer, codec._qs_buffer, w.flat] + [d.flat for d in state] + g16
        keep = [x.clone() for x in live]
        hyper, n0 = _lib.adam_hyper([HYPER["adamw"] + (1.0,)] * len(SHAPES)), ch.stub.psgd_stub_calls()
        with pytest.raises(ValueError, match="serves ranks 33-128"):
            plan.aggregate_comm_adam(c[0], c[1], c[2], c[3], hyper, 0, codec._comm, ch.stream, flat=inner._unc.plan,
                                     unc=u[0], unc_params=u[1], unc_ms=u[2], unc_vs=u[3], wide=True)
        with pytest.raises(ValueError, match="serves ranks 33-128"):
            plan.aggregate_mixed_comm_adam(c[4], c[0], c[5], c[1], c[2], c[3], hyper, 0, codec._comm, ch.stream,
                                           flat=inner._unc.plan, unc_bf16=u[4], unc_residual=u[0], unc_params_bf16=u[5],
                                           unc_masters=u[1], unc_ms=u[2], unc_vs=u[3], wide=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(live, keep))
        assert ch.stub.psgd_stub_calls() == n0
        inner.close()
    finally:
        ch.close()


def test_wide_entries_refuse_rank_32_and_touch_nothing(tmp_path):
    torch.multiprocessing.spawn(_refused, args=(_init(tmp_path),), nprocs=1, join=True)


# ------------------------------------------------------------------ adam_step / adam_master_step at rank 64
MODEL = [(96, 260), (130, 321), (100, 13), (50,)]  # rates 0.88 / 1.09 / 1.44 at rank 64, I = 2; the bias stays dense


def _setup(master):
    from powersgd_amd import Config, Fp32ResidualPowerSGD, PowerSGD

    gen = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to("cuda:0")) for s in MODEL]
    model = [torch.nn.Parameter(p.detach().bfloat16()) for p in params] if master else params
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-2, foreach=False)
    agg = (Fp32ResidualPowerSGD if master else PowerSGD)(model, Config(64, 0.5, 2, 1))
    assert (agg.inner if master else agg)._powersgd._plan.is_wide()
    return params, model, opt, agg


def _step(opt, agg, params, model, master, fused):
    from powersgd_amd import adam_master_step, adam_step, optimizer_step

    if fused:
        return adam_master_step(opt, agg, model) if master else adam_step(opt, agg)
    if not master:
        return optimizer_step(opt, agg)
    for p, a in zip(params, agg.aggregate_fp32([y.grad for y in model])):  # the unfused master sequence
        p.grad = a
    opt.step()
    for p, y in zip(params, model):
        p.grad = None
        y.data.copy_(p.data)


def _parity(_, initfile, master):
    from powersgd_amd import _lib, adam_master_step_applies, adam_step_applies

    torch.cuda.set_device(0)
    torch.distributed.init_process_group("nccl", init_method=f"file://{initfile}", rank=0, world_size=1,
                                         device_id=torch.device("cuda:0"))
    try:
        (pa, wa, oa, ga), (pb, wb, ob, gb) = _setup(master), _setup(master)
        seen = {}
        ob.register_step_pre_hook(lambda *_: seen.update(g=[p.grad.detach().clone() for p in pb]))
        for t in range(3):  # one warm-up step, then two compressing ones
            before = [[y.data.clone()] + [ob.state[y][k].clone() for k in KEYS] for y in pb] if t else None
            _backward(wa, t)
            for x, y in zip(wa, wb):
                y.grad = x.grad.clone()
            applies = adam_master_step_applies(oa, ga, wa) if master else adam_step_applies(oa, ga)
            assert applies == (t >= 1), (master, t)
            _step(oa, ga, pa, wa, master, True)
            _step(ob, gb, pb, wb, master, False)
            torch.cuda.synchronize()
            res = [(ga.residual, gb.residual)] if master else [(x.grad, y.grad) for x, y in zip(pa, pb)]
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in res), (master, t, "residual")
            for i, (x, y) in enumerate(zip(pa, pb)):
                sx, sy = oa.state[x], ob.state[y]
                assert sx["step"].device.type == "cpu" and float(sx["step"]) == float(sy["step"]) == t + 1, (t, i)
                if master:
                    assert torch.equal(_b16(wa[i].data), _b16(x.data.bfloat16())), (t, i, "model != bf16(master)")
                if t:
                    h = _lib.adam_hyper([(1e-3, 0.9, 0.999, 1e-8, 1e-2, True, float(t + 1))])[0]
                    _, bound = _ref64(h, seen["g"][i].cpu(), *(b.cpu() for b in before[i]))
                    got = [x.data.cpu()] + [sx[k].cpu() for k in KEYS]
                    want = [y.data.cpu().double()] + [sy[k].cpu().double() for k in KEYS]
                    _within(got, want, bound, (master, t, i), scale=2.0)
                x.data.copy_(y.data)  # identical state before the next step: bounds do not compound
                for k in KEYS:
                    sx[k].copy_(sy[k])
                if master:
                    wa[i].data.copy_(wb[i].data)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("master", [False, True])
def test_adam_steps_take_the_wide_entry_at_rank_64(master, tmp_path):
    """adam_step (adam_master_step) on a rank-64 plan in a one-rank process group: *_applies true on the compressing
    steps, the residual bitwise optimizer_step's (the unfused master sequence's), p / exp_avg / exp_avg_sq within
    2 x THE BOUND of torch's, state["step"] equal and on the CPU, the model bitwise bf16(master)."""
    torch.multiprocessing.spawn(_parity, args=(str(tmp_path / "init"), master), nprocs=1, join=True)
