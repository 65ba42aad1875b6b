"""The fused SGD step (include/psgd.h: psgd_sgd_update, psgd_aggregate_comm_sgd; powersgd_amd/sgd.py).

THE BOUND used below (derived, not measured). The update of one element is a chain of fp32
operations, each rounded on its own: wd*p, g + that (weight decay); mu*buf, cd*d, their sum
(momentum, not on a tensor's first step); mu*buf', d + that (nesterov); (-lr)*u, p + that. A
rounded operation returns its exact result times (1 + e), |e| <= 2^-24, so it adds at most 2^-24
times the magnitude of its own result, and every later operation passes an earlier error on
multiplied by one of |wd|, |mu|, |cd|, |lr| (all <= 1 here) or by 1 (an add). With S the sum of the
magnitudes of every intermediate (every operation's result; the inputs g, p, buf are exact and not
in it) of the formula evaluated in float64 on the same fp32 inputs and the same fp32-rounded
hyperparameters, the first-order error is at most 2^-24 * S; the k rounded operations of the path
(k <= 9) compound to at most (1 + 2^-24)^k - 1 of that beyond first order, and k * 2^-24 * S covers
both. buf' has its own, shorter chain (at most wd*p, g + that, mu*buf, cd*d, their sum: k <= 5) and
its own S over those results only; on a first step without weight decay buf' = g exactly (k = 0).

Two evaluations of the formula that each round every operation at most once (the kernels here; torch's,
which may contract a product into the following add, dropping a rounding) are each within 2^-24 * S
of the exact value to first order, so they differ by at most 2 * 2^-24 * S: within k * 2^-24 * S
whenever k >= 2, which holds on every path to p' (and to buf' wherever torch and the kernel can differ
at all). That is how sgd_step is compared with torch.optim.SGD below."""
import ctypes

import pytest
import torch

from test_gpu_comm_dst import NUMEL, SHAPES, STEPS, _bits, _Child, _Dst, _fresh, _init

pytestmark = pytest.mark.gpu
# (lr, momentum, dampening, weight_decay, nesterov)
HYPER = {"plain": (0.1, 0.0, 0.0, 0.0, False), "mom_wd": (0.1, 0.9, 0.0, 5e-4, False),
         "damp": (0.1, 0.9, 0.1, 0.0, False), "nesterov": (0.1, 0.9, 0.0, 5e-4, True)}


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _ref64(hp, first, g, p, b):
    """The formula of include/psgd.h in float64 on fp32 inputs: p', buf' (None without momentum), and
    per element the bounds k * 2^-24 * S of p' and of buf' (each its own chain's k and S)."""
    lr, mu, damp, wd, nest = hp
    lr, mu, cd, wd = _f32(lr), _f32(mu), _f32(1.0 - damp), _f32(wd)
    g, p, b = g.double(), p.double(), b.double()
    d, S, k = g, torch.zeros_like(g), 0
    if wd != 0:
        d = g + wd * p
        S, k = S + (wd * p).abs() + d.abs(), k + 2
    u, nb, Sb, kb = d, None, None, None
    if mu != 0:
        nb = d
        if not first:
            nb = mu * b + cd * d
            S, k = S + (mu * b).abs() + (cd * d).abs() + nb.abs(), k + 3
        Sb, kb = S.clone(), k  # buf' is done here: its own chain
        u = nb
        if nest:
            u = d + mu * nb
            S, k = S + (mu * nb).abs() + u.abs(), k + 2
    np_ = p - lr * u
    S, k = S + (lr * u).abs() + np_.abs(), k + 2
    return np_, nb, k * 2.0 ** -24 * S, None if nb is None else kb * 2.0 ** -24 * Sb


# ------------------------------------------------------------------ the element-wise kernel
LENGTHS = (1, 3, 4, 5, 4096, 4097, 8195)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("name", sorted(HYPER))
def test_sgd_update_against_float64(name, first):
    """k_sgd_update alone: every length x every offset (0, 1, 2 elements into a 16-byte aligned slot)
    of each of the three pointers, as the tensors of ONE launch; canaries round every tensor."""
    from powersgd_amd import _lib

    dev, hp = torch.device("cuda:0"), HYPER[name]
    cases = [(n, og, op, ob) for n in LENGTHS for og in range(3) for op in range(3) for ob in range(3)]
    slot = 8 + max(LENGTHS) + 8 + (-(16 + max(LENGTHS))) % 4  # canaries either side, a multiple of 4
    gen = torch.Generator().manual_seed(11)
    flat = {k: torch.full((len(cases) * slot,), float("nan")) for k in "gpb"}
    inside = {k: torch.zeros(len(cases) * slot, dtype=torch.bool) for k in "gpb"}
    views = {k: [] for k in "gpb"}
    for i, (n, og, op, ob) in enumerate(cases):
        for k, o in zip("gpb", (og, op, ob)):
            lo = i * slot + 8 + o
            flat[k][lo:lo + n] = torch.randn(n, generator=gen)
            inside[k][lo:lo + n] = True
            views[k].append((lo, n))
    devb = {k: flat[k].to(dev) for k in "gpb"}
    assert all(devb[k].data_ptr() % 16 == 0 for k in "gpb")
    ptrs = {k: _lib.ptr_array([devb[k].data_ptr() + 4 * lo for lo, _ in views[k]]) for k in "gpb"}
    hyper = _lib.sgd_hyper([hp + (first,)] * len(cases))
    _lib.sgd_update(None, ctypes.addressof(ptrs["g"]), ctypes.addressof(ptrs["p"]), ctypes.addressof(ptrs["b"]),
                    [n for n, *_ in cases], hyper, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out = {k: devb[k].cpu() for k in "gpb"}
    for k in "gpb":  # canaries, and g is read only
        keep = ~inside[k] if k != "g" else torch.ones_like(inside[k])
        assert torch.equal(_bits(out[k])[keep], _bits(flat[k])[keep]), (k, "outside the tensors")
    if hp[1] == 0:
        assert torch.equal(_bits(out["b"]), _bits(flat["b"])), "buf is neither read nor written without momentum"
    worst = worst_b = 0.0
    for (n, og, op, ob), (lg, _), (lp, _), (lb, _) in zip(cases, views["g"], views["p"], views["b"]):
        want_p, want_b, bound, bound_b = _ref64(hp, first, flat["g"][lg:lg + n], flat["p"][lp:lp + n],
                                                flat["b"][lb:lb + n])
        ep = (out["p"][lp:lp + n].double() - want_p).abs()
        worst = max(worst, float((ep / bound).max()))
        assert bool((ep <= bound).all()), (n, og, op, ob, float((ep / bound).max()))
        if want_b is not None:
            eb = (out["b"][lb:lb + n].double() - want_b).abs()
            worst_b = max(worst_b, float((eb / bound_b.clamp_min(1e-300)).max()))
            assert bool((eb <= bound_b).all()), (n, og, op, ob, "buf", worst_b)
    print(f"sgd_update {name} first={first}: worst error / bound = {worst:.3f} (p), {worst_b:.3f} (buf)")


# ------------------------------------------------------------------ the fused entry against its definition
PAIRS = (("aligned", "aligned"), ("one_in", "one_in"), ("aligned", "one_in"))


def _run(ch, rank, iters, hp, fused, places=("aligned", "aligned"), comm=True):
    """STEPS steps of psgd_aggregate_comm_sgd (`fused`) or of its defining sequence; None where the
    plan is not admitted (after checking that the call refuses and touches nothing)."""
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import _psgd_host

    grads, views, inner = ch.codec(rank, iters)
    codec, plan = inner._powersgd, inner._powersgd._plan
    mom = hp[1] != 0
    P, B = _Dst(places[0], ch.dev), _Dst(places[1], ch.dev)
    gen = torch.Generator().manual_seed(77)
    for v in P.views:
        v.copy_(torch.randn(v.shape, generator=gen))
    for v in B.views:
        v.zero_()
    scratch = _Dst("aligned", ch.dev)
    mask = inner.is_compressed_mask
    tabs = [_psgd_host.PtrTable([list(s) for s in SHAPES], mask, _lib.PSGD_F32, 0) for _ in range(3)]
    order = [i for i, c in enumerate(mask) if c] + [i for i, c in enumerate(mask) if not c]
    ok = plan.sgd_ok(0, ch.world)
    assert ok == plan.sgd_ok(1, ch.world) and plan.dst_ok(0, ch.world) >= ok
    rec = []
    for t in range(STEPS):
        for v, g in zip(views, _fresh(t)):
            v.add_(g.to(ch.dev))
        hyper = _lib.sgd_hyper([hp + (t == 0,)] * len(SHAPES))
        n0 = ch.stub.psgd_stub_calls()
        inner._table.fill(views)
        for tab, d in zip(tabs, (P, B, scratch)):
            tab.fill(d.views)
        kw = dict(flat=inner._unc.plan, unc=inner._table.unc_addr())
        if fused or not ok:
            call = lambda: plan.aggregate_comm_sgd(  # noqa: E731
                inner._table.comp_addr(), tabs[0].comp_addr(), tabs[1].comp_addr() if mom else None, hyper,
                codec.step_counter, codec._comm if comm else None, ch.stream, unc_params=tabs[0].unc_addr(),
                unc_bufs=tabs[1].unc_addr() if mom else None, **kw)
            if not ok:
                live = [grads, P.flat, B.flat, codec._ps_buffer, codec._qs_buffer]
                keep = [x.clone() for x in live]
                with pytest.raises(ValueError, match="no admitted update instance"):
                    call()
                torch.cuda.synchronize()
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(live, keep)) and ch.stub.psgd_stub_calls() == n0
                inner.close()
                return None
            call()
        else:
            plan.aggregate_comm_dst(inner._table.comp_addr(), tabs[2].comp_addr(), codec.step_counter, codec._comm,
                                    ch.stream, unc_dst=tabs[2].unc_addr(), **kw)
            arr = [_lib.ptr_array([d.views[i].data_ptr() for i in order]) for d in (scratch, P, B)]
            g_, p_, b_ = (ctypes.addressof(a) for a in arr)
            _lib.sgd_update(plan, g_, p_, b_ if mom else None, [NUMEL[i] for i in order], hyper, ch.stream)
        codec.step_counter += 1
        torch.cuda.synchronize()
        rec.append({"calls": ch.stub.psgd_stub_calls() - n0, "p": [_bits(v).cpu() for v in P.views],
                    "buf": [_bits(v).cpu() for v in B.views], "residual": _bits(grads).cpu(),
                    "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu(),
                    "canary": P.canary_intact() and B.canary_intact()})
    inner.close()
    return rec


def _fused(_, init, world, ranks):
    ch = _Child(init, world)
    try:
        for rank in ranks:
            for iters in (1, 2, 3):
                for name in ("plain", "mom_wd"):
                    ref = _run(ch, rank, iters, HYPER[name], False)  # once per case, shared by the placements
                    if ref is None:  # not admitted: refused, nothing touched; only where the issue allows it
                        assert rank == 32 or (rank == 8 and iters in (2, 3)), (world, rank, iters)
                        continue
                    assert [r["calls"] for r in ref] == [iters + 1] * STEPS
                    # at one rank also without a communicator: the same kernels, no collective
                    for places, comm in [(pl, True) for pl in PAIRS] + ([(PAIRS[1], False)] if world == 1 else []):
                        one = _run(ch, rank, iters, HYPER[name], True, places, comm)
                        for t, (x, y) in enumerate(zip(one, ref)):
                            ctx = (world, rank, iters, name, places, comm, t)
                            for k in ("p", "buf"):
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
    """psgd_aggregate_comm_sgd against psgd_aggregate_comm_dst + psgd_sgd_update: raw bits of every p,
    buf, residual, P/Q state and the collective count after each of four steps."""
    torch.multiprocessing.spawn(_fused, args=(_init(tmp_path), world, ranks), nprocs=1, join=True)


# ------------------------------------------------------------------ sgd_step against optimizer_step
MODEL = [(32, 16, 3, 3), (64, 32), (48, 24), (32,), (3, 100)]


def _setup(dtype=torch.float32, max_grad_norm=None, start=1, **opt_kw):
    from powersgd_amd import Config, PowerSGD

    gen = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to("cuda:0", dtype)) for s in MODEL]
    opt = torch.optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=5e-4, **opt_kw)
    agg = PowerSGD(params, Config(rank=2, min_compression_rate=2, num_iters_per_step=2,
                                  start_compressing_after_num_steps=start), max_grad_norm=max_grad_norm)
    return params, opt, agg


def _backward(params, t):
    gen = torch.Generator().manual_seed(500 + t)
    for p in params:
        g = torch.randn(p.shape, generator=gen).to(p.device, p.dtype)
        p.grad = g if p.grad is None else p.grad + g


def _step_parity(_, initfile):
    from powersgd_amd import optimizer_step, sgd_step, sgd_step_applies

    pa, oa, ga = _setup()
    for p in pa:
        p.grad = torch.zeros_like(p)
    ga.step_counter = 1  # past the warm-up step
    assert not sgd_step_applies(oa, ga)
    # no process group: optimizer_step runs the world-size-1 step (fused final kernels), whose residual
    # rounds differently from the communicator sequence's, so sgd_step keeps optimizer_step there
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("nccl", init_method=f"file://{initfile}", rank=0, world_size=1,
                                         device_id=torch.device("cuda:0"))
    try:
        _parity_body(optimizer_step, sgd_step, sgd_step_applies)
    finally:
        torch.distributed.destroy_process_group()


def test_sgd_step_against_optimizer_step(tmp_path):
    """Three steps from identical state in a one-rank process group over the library's communicator,
    with one warm-up step and with none (sgd_step creates the momentum buffers: `first`): p.grad bitwise
    the same residual; parameters and momentum buffers of sgd_step and of optimizer_step +
    torch.optim.SGD within THE BOUND of each other and of the float64 formula on the averages torch's
    optimizer was handed; maximize, a bf16 model and max_grad_norm keep optimizer_step bit for bit."""
    torch.multiprocessing.spawn(_step_parity, args=(str(tmp_path / "init"),), nprocs=1, join=True)


def _parity_body(optimizer_step, sgd_step, sgd_step_applies):
    for start in (1, 0):  # one warm-up step (torch creates the buffers); none (sgd_step does: `first`)
        pa, oa, ga = _setup(start=start)
        pb, ob, gb = _setup(start=start)
        seen = {}
        ob.register_step_pre_hook(lambda *_: seen.update(g=[p.grad.detach().clone() for p in pb]))
        for t in range(3):
            for x, y in zip(pa, pb):  # identical state before every step
                x.data.copy_(y.data)
                if "momentum_buffer" in ob.state[y]:
                    oa.state[x]["momentum_buffer"] = ob.state[y]["momentum_buffer"].clone()
            before = [(y.data.clone(), ob.state[y]["momentum_buffer"].clone() if ob.state[y] else None) for y in pb]
            _backward(pa, t)
            _backward(pb, t)
            assert sgd_step_applies(oa, ga) == (t >= start), (start, t)
            sgd_step(oa, ga)
            optimizer_step(ob, gb)
            torch.cuda.synchronize()
            for i, (x, y) in enumerate(zip(pa, pb)):
                ctx = (start, t, i)
                assert torch.equal(_bits(x.grad), _bits(y.grad)), (ctx, "residual")
                p0, b0 = before[i]
                first = b0 is None
                want_p, want_b, bound, bound_b = _ref64((0.1, 0.9, 0.0, 5e-4, False), first, seen["g"][i].cpu(), p0.cpu(),
                                                        torch.zeros_like(p0).cpu() if first else b0.cpu())
                bx, by = (o.state[q]["momentum_buffer"].cpu().double() for o, q in ((oa, x), (ob, y)))
                px, py = x.data.cpu().double(), y.data.cpu().double()
                # sgd_step against optimizer_step + torch.optim.SGD, directly (module docstring)
                assert bool(((px - py).abs() <= bound).all()), (ctx, "p", float(((px - py).abs() / bound).max()))
                assert bool(((bx - by).abs() <= bound_b).all()), (ctx, "buf", float(((bx - by).abs() / bound_b).max()))
                for who, pp, bb in (("sgd_step", px, bx), ("torch", py, by)):  # and each against float64
                    assert bool(((pp - want_p).abs() <= bound).all()), (ctx, who)
                    assert bool(((bb - want_b).abs() <= bound_b).all()), (ctx, who, "buf")
    for kw in (dict(maximize=True), dict(dtype=torch.bfloat16), dict(max_grad_norm=1.0)):  # these keep optimizer_step
        pa, oa, ga = _setup(**kw)
        pb, ob, gb = _setup(**kw)
        for t in range(3):
            _backward(pa, t)
            _backward(pb, t)
            assert not sgd_step_applies(oa, ga), kw
            sgd_step(oa, ga)
            optimizer_step(ob, gb)
        torch.cuda.synchronize()
        for x, y in zip(pa, pb):
            assert torch.equal(x.data, y.data) and torch.equal(x.grad, y.grad), kw
            assert torch.equal(oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"]), kw
