"""The fused Adam / AdamW step (include/psgd.h: psgd_adam_update, psgd_aggregate_comm_adam;
powersgd_amd/adam.py).

THE BOUND used below (derived, not measured): a forward first-order propagation carried beside the
float64 evaluation of the formula on the same fp32 inputs and the same fp32-rounded record, with
u = 2^-24. Inputs and the record are exact. Each fp32 operation returns its exact result times
(1 + e), |e| <= u, so a rounded result x adds u|x| to the error it inherits; an add inherits
e_a + e_b; a multiply by a record scalar c inherits |c| e_a; (w2 d) d inherits 2|d| e_d beside its
two roundings (u|w2 d||d| and u|w2 d d|; w2 <= 1); sqrt inherits e_v / (2 sqrt(v')) where v' > 0 and
sqrt(e_v) at v' = 0 (|sqrt(x) - 0| <= sqrt(e_v) for 0 <= x <= e_v); a / b inherits
e_a / |b| + |a| e_b / b^2. The chain in order: wd p, g + that (coupled) or decay p (decoupled);
d - m; w1 (d - m), m + that (or (1 - w1)(d - m), d - that: 1 - w1 is exact in fp32 for w1 >= 0.5,
Sterbenz); beta2 v, w2 d, (w2 d) d, their sum; sqrt, / bc2_sqrt, + eps; m' / den; step_size times
that; p0 minus that: at most 14 rounded operations on the path to p', so the terms beyond first order
are below 14 u relative and the total is scaled by (1 + 2^-10). m' and v' carry the bounds of their
own, shorter chains.

Two evaluations that each round every operation at most once (the kernels here; torch's, which may
contract a product into the following add, dropping a rounding) are each within THE BOUND of the
exact value, so they differ by at most 2 x THE BOUND: that is how adam_step is compared with torch."""
import ctypes

import pytest
import torch

from test_gpu_comm_dst import NUMEL, SHAPES, STEPS, _bits, _Child, _Dst, _fresh, _init

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# (lr, beta1, beta2, eps, weight_decay, decoupled)
HYPER = {"plain": (1e-3, 0.9, 0.999, 1e-8, 0.0, False), "adam_l2": (1e-3, 0.9, 0.999, 1e-8, 1e-2, False),
         "adamw": (1e-3, 0.9, 0.999, 1e-8, 1e-2, True), "lerp_hi": (1e-3, 0.4, 0.999, 1e-8, 0.0, False)}


def _ref64(h, g, p, m, v):
    """(p', m', v') of the formula in float64 under record `h` (an AdamHyper), and THE BOUND of each."""
    g, p, m, v = (x.double() for x in (g, p, m, v))
    rnd = lambda x, e=0.0: e + U * x.abs()  # noqa: E731  a rounded result: inherited error + u|x|
    d, e_d, p0, e_p0 = g, torch.zeros_like(g), p, torch.zeros_like(p)
    if h.weight_decay != 0 and h.decoupled:
        p0 = h.decay * p
        e_p0 = rnd(p0)
    elif h.weight_decay != 0:
        t = h.weight_decay * p
        d = g + t
        e_d = rnd(d, rnd(t))
    dm = d - m
    e_dm = rnd(dm, e_d)
    if h.w1 < 0.5:
        t = h.w1 * dm
        nm = m + t
        e_m = rnd(nm, rnd(t, h.w1 * e_dm))
    else:
        t = (1.0 - h.w1) * dm
        nm = d - t
        e_m = rnd(nm, e_d + rnd(t, (1.0 - h.w1) * e_dm))
    a, b1 = h.beta2 * v, h.w2 * d
    b2 = b1 * d
    nv = a + b2
    e_v = rnd(nv, rnd(a) + rnd(b2, 2 * d.abs() * e_d + d.abs() * rnd(b1)))
    s = nv.sqrt()
    e_s = rnd(s, torch.where(nv > 0, e_v / (2 * s).clamp_min(1e-300), e_v.sqrt()))
    q = s / h.bc2_sqrt
    den = q + h.eps
    e_den = rnd(den, rnd(q, e_s / h.bc2_sqrt))
    r = nm / den
    e_r = rnd(r, e_m / den.abs() + nm.abs() * e_den / den ** 2)
    t = h.step_size * r
    np_ = p0 - t
    e_p = rnd(np_, e_p0 + rnd(t, h.step_size * e_r))
    k = 1 + 2.0 ** -10
    return (np_, nm, nv), (k * e_p, k * e_m, k * e_v)


def _within(got, want, bound, ctx, scale=1.0):
    """The worst error / bound over p', m', v' after asserting each within scale x its bound."""
    worst = 0.0
    for name, x, w, b in zip("pmv", got, want, bound):
        err = (x.double() - w).abs()
        assert bool((err <= scale * b).all()), (ctx, name, float((err / b.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / b.clamp_min(1e-300)).max()))
    return worst


# ------------------------------------------------------------------ the element-wise kernel
LENGTHS = (1, 3, 4, 5, 4096, 4097, 8195)


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("name", sorted(HYPER))
def test_adam_update_against_float64(name, t):
    """k_adam_update alone: every length x offsets 0 / 1 / 2 elements of g and p and 0 / 1 of m and v (into
    16-byte aligned slots), as the tensors of ONE launch; NaN canaries round every tensor; exact zeros in
    g, m and v (den = eps)."""
    from powersgd_amd import _lib

    dev = torch.device("cuda:0")
    cases = [(n, og, op, om, ov) for n in LENGTHS for og in range(3) for op in range(3) for om in range(2)
             for ov in range(2)]
    slot = 8 + max(LENGTHS) + 8 + (-(16 + max(LENGTHS))) % 4  # canaries either side, a multiple of 4
    gen = torch.Generator().manual_seed(11)
    flat = {k: torch.full((len(cases) * slot,), float("nan")) for k in "gpmv"}
    inside = {k: torch.zeros(len(cases) * slot, dtype=torch.bool) for k in "gpmv"}
    views = {k: [] for k in "gpmv"}
    for i, (n, *offs) in enumerate(cases):
        zero = torch.rand(n, generator=gen) < 0.125  # the first-step state: g, m and v all exactly zero
        for k, o in zip("gpmv", offs):
            x = torch.randn(n, generator=gen)
            x = x * x if k == "v" else x
            lo = i * slot + 8 + o
            flat[k][lo:lo + n] = x if k == "p" else torch.where(zero, torch.zeros(()), x)
            inside[k][lo:lo + n] = True
            views[k].append(lo)
    devb = {k: flat[k].to(dev) for k in "gpmv"}
    assert all(devb[k].data_ptr() % 16 == 0 for k in "gpmv")
    ptrs = {k: _lib.ptr_array([devb[k].data_ptr() + 4 * lo for lo in views[k]]) for k in "gpmv"}
    hyper = _lib.adam_hyper([HYPER[name] + (float(t),)] * len(cases))
    _lib.adam_update(None, *(ctypes.addressof(ptrs[k]) for k in "gpmv"), [c[0] for c in cases], hyper,
                     torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out = {k: devb[k].cpu() for k in "gpmv"}
    for k in "gpmv":  # canaries, and g is read only
        keep = ~inside[k] if k != "g" else torch.ones_like(inside[k])
        assert torch.equal(_bits(out[k])[keep], _bits(flat[k])[keep]), (k, "outside the tensors")
    worst = 0.0
    for i, case in enumerate(cases):
        cut = lambda src: [src[k][views[k][i]:views[k][i] + case[0]] for k in "gpmv"]  # noqa: E731
        want, bound = _ref64(hyper[0], *cut(flat))
        worst = max(worst, _within(cut(out)[1:], want, bound, case))
    print(f"adam_update {name} t={t}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------ the fused entry against its definition
PLACES = (("aligned",) * 3, ("one_in",) * 3, ("aligned", "aligned", "one_in"))  # of p, m, v; the last: element form
NOT_ADMITTED = {(8, 2), (8, 3)}  # (rank, I) recorded as not admitted in profiles/adam_step/resources.txt


def _run(ch, rank, iters, hp, fused, places=PLACES[0], comm=True):
    """STEPS steps of psgd_aggregate_comm_adam (`fused`) or of its defining sequence; None where the
    plan is not admitted (after checking that the call refuses and touches nothing)."""
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import _psgd_host

    grads, views, inner = ch.codec(rank, iters)
    codec, plan = inner._powersgd, inner._powersgd._plan
    state = [_Dst(pl, ch.dev) for pl in places]  # p, m, v
    gen = torch.Generator().manual_seed(77)
    for x in state[0].views:
        x.copy_(torch.randn(x.shape, generator=gen))
    for d in state[1:]:
        for x in d.views:
            x.zero_()
    scratch = _Dst("aligned", ch.dev)
    mask = inner.is_compressed_mask
    tabs = [_psgd_host.PtrTable([list(s) for s in SHAPES], mask, _lib.PSGD_F32, 0) for _ in range(4)]
    order = [i for i, c in enumerate(mask) if c] + [i for i, c in enumerate(mask) if not c]
    ok = plan.adam_ok(0, ch.world)
    assert ok == plan.adam_ok(1, ch.world) and plan.dst_ok(0, ch.world) >= ok
    rec = []
    for t in range(STEPS):
        for x, g in zip(views, _fresh(t)):
            x.add_(g.to(ch.dev))
        hyper = _lib.adam_hyper([hp + (float(t + 1),)] * len(SHAPES))
        n0 = ch.stub.psgd_stub_calls()
        inner._table.fill(views)
        for tab, d in zip(tabs, state + [scratch]):
            tab.fill(d.views)
        kw = dict(flat=inner._unc.plan, unc=inner._table.unc_addr())
        if fused or not ok:
            call = lambda: plan.aggregate_comm_adam(  # noqa: E731
                inner._table.comp_addr(), *(tab.comp_addr() for tab in tabs[:3]), hyper, codec.step_counter,
                codec._comm if comm else None, ch.stream, unc_params=tabs[0].unc_addr(), unc_ms=tabs[1].unc_addr(),
                unc_vs=tabs[2].unc_addr(), **kw)
            if not ok:
                live = [grads, codec._ps_buffer, codec._qs_buffer] + [d.flat for d in state]
                keep = [x.clone() for x in live]
                with pytest.raises(ValueError, match="no admitted update instance"):
                    call()
                torch.cuda.synchronize()
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(live, keep)) and ch.stub.psgd_stub_calls() == n0
                inner.close()
                return None
            call()
        else:
            plan.aggregate_comm_dst(inner._table.comp_addr(), tabs[3].comp_addr(), codec.step_counter, codec._comm,
                                    ch.stream, unc_dst=tabs[3].unc_addr(), **kw)
            arr = [_lib.ptr_array([d.views[i].data_ptr() for i in order]) for d in [scratch] + state]
            _lib.adam_update(plan, *(ctypes.addressof(a) for a in arr), [NUMEL[i] for i in order], hyper, ch.stream)
        codec.step_counter += 1
        torch.cuda.synchronize()
        rec.append({"calls": ch.stub.psgd_stub_calls() - n0, "residual": _bits(grads).cpu(),
                    "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu(),
                    "canary": all(d.canary_intact() for d in state),
                    **{k: [_bits(x).cpu() for x in d.views] for k, d in zip("pmv", state)}})
    inner.close()
    return rec


def _fused(_, init, world, ranks):
    ch = _Child(init, world)
    try:
        for rank in ranks:
            for iters in (1, 2, 3):
                for name in ("adam_l2", "adamw"):
                    ref = _run(ch, rank, iters, HYPER[name], False)  # once per case, shared by the placements
                    if ref is None:  # not admitted: refused, nothing touched; the coverage cap of the issue
                        assert (rank, iters) in NOT_ADMITTED and not (rank in (1, 2, 4) and iters in (1, 2)), (world, rank, iters)
                        continue
                    assert [r["calls"] for r in ref] == [iters + 1] * STEPS
                    # at one rank also without a communicator: the same kernels, no collective
                    for places, comm in [(pl, True) for pl in PLACES] + ([(PLACES[1], False)] if world == 1 else []):
                        one = _run(ch, rank, iters, HYPER[name], True, places, comm)
                        for t, (x, y) in enumerate(zip(one, ref)):
                            ctx = (world, rank, iters, name, places, comm, t)
                            for k in "pmv":
                                assert all(torch.equal(a, b) for a, b in zip(x[k], y[k])), (ctx, k)
                            for k in ("residual", "ps", "qs"):
                                assert torch.equal(x[k], y[k]), (ctx, k)
                            assert x["calls"] == (y["calls"] if comm else 0), (ctx, "collective count")
                            assert x["canary"], ctx
    finally:
        ch.close()


@pytest.mark.parametrize("ranks", [(1, 2), (4, 8), (16, 32)])
@pytest.mark.parametrize("world", [3, 1])
def test_fused_entry_equals_its_definition_bitwise(world, ranks, tmp_path):
    """psgd_aggregate_comm_adam against psgd_aggregate_comm_dst + psgd_adam_update: raw bits of every p, m,
    v, residual, P/Q state and the collective count after each step."""
    torch.multiprocessing.spawn(_fused, args=(_init(tmp_path), world, ranks), nprocs=1, join=True)


# ------------------------------------------------------------------ adam_step against optimizer_step
MODEL = [(32, 16, 3, 3), (64, 32), (48, 24), (32,), (3, 100)]
KEYS = ("exp_avg", "exp_avg_sq")


def _setup(cls, **opt_kw):
    from powersgd_amd import Config, PowerSGD

    gen = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to("cuda:0")) for s in MODEL]
    opt = cls(params, lr=1e-3, weight_decay=1e-2, foreach=False, **opt_kw)
    agg = PowerSGD(params, Config(rank=2, min_compression_rate=2, num_iters_per_step=2,
                                  start_compressing_after_num_steps=1))
    return params, opt, agg


def _backward(params, t):
    gen = torch.Generator().manual_seed(500 + t)
    for p in params:
        g = torch.randn(p.shape, generator=gen).to(p.device, p.dtype)
        p.grad = g if p.grad is None else p.grad + g


def _step_parity(_, initfile):
    from powersgd_amd import _lib, adam_step, adam_step_applies, optimizer_step

    torch.cuda.set_device(0)
    torch.distributed.init_process_group("nccl", init_method=f"file://{initfile}", rank=0, world_size=1,
                                         device_id=torch.device("cuda:0"))
    try:
        for cls in (torch.optim.AdamW, torch.optim.Adam):
            pa, oa, ga = _setup(cls)
            pb, ob, gb = _setup(cls)
            seen = {}
            ob.register_step_pre_hook(lambda *_: seen.update(g=[p.grad.detach().clone() for p in pb]))
            for t in range(4):  # one warm-up step, then three compressing ones
                before = [[y.data.clone()] + [ob.state[y][k].clone() for k in KEYS] for y in pb] if t else None
                _backward(pa, t)
                _backward(pb, t)
                assert adam_step_applies(oa, ga) == (t >= 1), (cls, t)
                adam_step(oa, ga)
                optimizer_step(ob, gb)
                torch.cuda.synchronize()
                for i, (x, y) in enumerate(zip(pa, pb)):
                    ctx = (cls.__name__, t, i)
                    assert torch.equal(_bits(x.grad), _bits(y.grad)), (ctx, "residual")
                    sx, sy = oa.state[x], ob.state[y]
                    assert sx["step"].device.type == "cpu" and float(sx["step"]) == float(sy["step"]) == t + 1, ctx
                    if t:
                        h = _lib.adam_hyper([(1e-3, 0.9, 0.999, 1e-8, 1e-2, cls is torch.optim.AdamW, float(t + 1))])[0]
                        _, bound = _ref64(h, seen["g"][i].cpu(), *(b.cpu() for b in before[i]))
                        got = [x.data.cpu()] + [sx[k].cpu() for k in KEYS]
                        want = [y.data.cpu().double()] + [sy[k].cpu().double() for k in KEYS]
                        _within(got, want, bound, ctx, scale=2.0)
                    x.data.copy_(y.data)  # identical state before the next step: bounds do not compound
                    for k in KEYS:
                        sx[k].copy_(sy[k])
        # one optimizer_step between two adam_step calls: the shared state dict keeps working
        pa, oa, ga = _setup(torch.optim.AdamW)
        for t, step in enumerate((optimizer_step, adam_step, optimizer_step, adam_step)):
            _backward(pa, t)
            step(oa, ga)
        torch.cuda.synchronize()
        assert all(float(oa.state[x]["step"]) == 4 and bool(torch.isfinite(x).all()) for x in pa)
    finally:
        torch.distributed.destroy_process_group()


def test_adam_step_against_optimizer_step(tmp_path):
    """AdamW and coupled Adam (foreach=False) in a one-rank process group over the library's communicator,
    one warm-up step then three compressing ones from identical state: p.grad bitwise the same residual,
    p / exp_avg / exp_avg_sq within 2 x THE BOUND of torch's, state["step"] equal and on the CPU."""
    torch.multiprocessing.spawn(_step_parity, args=(str(tmp_path / "init"),), nprocs=1, join=True)
