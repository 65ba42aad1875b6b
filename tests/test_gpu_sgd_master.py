"""The fused SGD step of a bf16 model with fp32 master weights (include/psgd.h: psgd_sgd_update_mp,
psgd_aggregate_mixed_comm_sgd[_wide]; powersgd_amd/sgd_master.py). THE BOUND is test_gpu_sgd_step.py's,
derived in its docstring; the bf16 weights have no tolerance: w == bf16(stored fp32 p'), raw bits; the
entries are DEFINED as a sequence of plain calls, so test 2 compares raw bits too."""
import ctypes

import pytest
import torch

from test_gpu_comm_dst import CANARY, SHAPES, _bits, _Child, _init, _mcr
from test_gpu_sgd_step import HYPER, _ref64
from test_gpu_sgd_wide import MODEL

pytestmark = pytest.mark.gpu
W_CANARY = 0x7FC1  # a bf16 quiet NaN with a payload


def _b16(x):
    return x.contiguous().view(torch.int16)


# ------------------------------------------------------------------ test 1: the element-wise kernel
LENGTHS = (1, 3, 4, 5, 4096, 4097)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("name", sorted(HYPER))
def test_sgd_update_mp_against_float64(name, first):
    """k_sgd_update_mp alone, every case a tensor of ONE launch: p' and buf' within THE BOUND of float64, w
    bitwise bf16(p'), NaN canaries round every tensor intact, g unchanged, buf untouched without momentum.
    Offsets (0,0,0 | 0) and (1,1,1 | 1) take the vector form (without momentum buf's offset is not looked
    at), every other case the element form."""
    from powersgd_amd import _lib

    dev, hp = torch.device("cuda:0"), HYPER[name]
    cases = [(n, og, op, ob, ow) for n in LENGTHS for og in (0, 1) for op in (0, 1) for ob in (0, 1) for ow in (0, 1, 2)]
    slot = 8 + max(LENGTHS) + 8 + (-(16 + max(LENGTHS))) % 4  # canaries either side, a multiple of 4 elements
    gen = torch.Generator().manual_seed(11)
    flat = {k: torch.full((len(cases) * slot,), float("nan")) for k in "gpb"}
    lo = {k: [i * slot + 8 + c[1 + j] for i, c in enumerate(cases)] for j, k in enumerate("gpbw")}
    for i, c in enumerate(cases):
        for k in "gpb":
            flat[k][lo[k][i]:lo[k][i] + c[0]] = torch.randn(c[0], generator=gen)
    devb = {k: flat[k].to(dev) for k in "gpb"}
    devb["w"] = torch.full((len(cases) * slot,), W_CANARY, dtype=torch.int16, device=dev)
    assert all(devb[k].data_ptr() % 16 == 0 for k in "gpbw")
    ptrs = {k: _lib.ptr_array([devb[k].data_ptr() + devb[k].element_size() * o for o in lo[k]]) for k in "gpbw"}
    hyper = _lib.sgd_hyper([hp + (first,)] * len(cases))
    _lib.sgd_update_mp(None, *(ctypes.addressof(ptrs[k]) for k in "gpbw"), [c[0] for c in cases], hyper,
                       torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out = {k: devb[k].cpu() for k in "gpbw"}
    assert torch.equal(_bits(out["g"]), _bits(flat["g"])), "g is read only"
    if hp[1] == 0:
        assert torch.equal(_bits(out["b"]), _bits(flat["b"])), "buf is neither read nor written without momentum"
    inside = {k: torch.zeros(len(cases) * slot, dtype=torch.bool) for k in "pbw"}
    worst = 0.0
    for i, c in enumerate(cases):
        old, new = ([src[k][lo[k][i]:lo[k][i] + c[0]] for k in "gpb"] for src in (flat, out))
        want_p, want_b, bound, bound_b = _ref64(hp, first, *old)
        ep = (new[1].double() - want_p).abs()
        assert bool((ep <= bound).all()), (c, "p", float((ep / bound).max()))
        worst = max(worst, float((ep / bound).max()))
        if want_b is not None:
            assert bool(((new[2].double() - want_b).abs() <= bound_b).all()), (c, "buf")
        w = out["w"][lo["w"][i]:lo["w"][i] + c[0]]
        assert torch.equal(w, _b16(new[1].bfloat16())), (c, "w != bf16(p')")
        for k in "pbw":
            inside[k][lo[k][i]:lo[k][i] + c[0]] = True
    for k in "pb":
        assert torch.equal(_bits(out[k])[~inside[k]], _bits(flat[k])[~inside[k]]), (k, "canary")
    assert bool((out["w"][~inside["w"]] == W_CANARY).all()), "w canary"
    print(f"sgd_update_mp {name} first={first}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------ test 2: the entries against their definitions
class _Buf:
    """Tensors of `shapes` in one bucket-like buffer, canary everywhere else: every view 16-byte aligned, or
    `shift` elements in."""

    def __init__(self, shapes, dtype, shift, dev):
        raw, self.canary = (torch.int32, CANARY) if dtype == torch.float32 else (torch.int16, W_CANARY)
        numel, offs, off = [torch.Size(s).numel() for s in shapes], [], 8
        for n in numel:
            off += (-off) % 8 + 8
            offs.append(off + shift)
            off += shift + n
        self.flat = torch.full((off + 8,), self.canary, dtype=raw, device=dev)
        self.views = [self.flat[o:o + n].view(dtype).view(s) for o, n, s in zip(offs, numel, shapes)]
        assert all(v.data_ptr() % 16 == shift * v.element_size() for v in self.views)
        self.outside = torch.ones(off + 8, dtype=torch.bool, device=dev)
        for o, n in zip(offs, numel):
            self.outside[o:o + n] = False

    def intact(self):
        return bool((self.flat[self.outside] == self.canary).all())


def _run(ch, shapes, rank, iters, hp, fused, shift=0, comm=True, steps=3):
    """`steps` steps of psgd_aggregate_mixed_comm_sgd[_wide] (`fused`) or of the defining sequence: the ADD,
    psgd_aggregate_comm_dst into scratch (a wide plan: psgd_aggregate_comm into slabs), psgd_sgd_update_mp.
    A plan that is not admitted: asserts that the call refuses and touches nothing, returns None."""
    from powersgd_amd import Config, PowerSGD, _lib
    from powersgd_amd.powersgd import _psgd_host

    numel, n, wide, mom = [torch.Size(s).numel() for s in shapes], len(shapes), rank > 32, hp[1] != 0
    residual = torch.zeros(sum(numel), device=ch.dev)
    views = [x.view(s) for x, s in zip(residual.split(numel), shapes)]
    inner = PowerSGD(views, Config(rank, 0.5 if wide else _mcr(rank, iters), iters, 0))
    codec, plan = inner._powersgd, inner._powersgd._plan
    codec._comm = ch.comm()
    assert plan.is_wide() == wide and inner._unc is not None
    P, B, scratch = (_Buf(shapes, torch.float32, 0, ch.dev) for _ in range(3))
    w = _Buf(shapes, torch.bfloat16, shift, ch.dev)
    gen = torch.Generator().manual_seed(77)
    for x, b in zip(P.views, B.views):
        x.copy_(torch.randn(x.shape, generator=gen))
        b.zero_()
    b0 = B.flat.clone()
    g16 = [torch.zeros(s, dtype=torch.bfloat16, device=ch.dev) for s in shapes]
    mask = inner.is_compressed_mask
    f32 = [_psgd_host.PtrTable([list(s) for s in shapes], mask, _lib.PSGD_F32, 0) for _ in range(3)]
    b16 = [_psgd_host.PtrTable([list(s) for s in shapes], mask, _lib.PSGD_BF16, 0) for _ in range(2)]
    add = _lib.Runs([0] * n, list(range(n)), [0] * n, numel, n, _lib.PSGD_F32, _lib.PSGD_BF16, source=list(range(n)), nsources=n)
    ws = torch.empty(add.workspace_bytes(), dtype=torch.uint8, device=ch.dev)
    add.bind(0, ws.data_ptr())
    order = [i for i, c in enumerate(mask) if c] + [i for i, c in enumerate(mask) if not c]
    query, other = (plan.mixed_sgd_wide_ok, plan.mixed_sgd_ok) if wide else (plan.mixed_sgd_ok, plan.mixed_sgd_wide_ok)
    ok = query(0, ch.world)
    assert ok == query(1, ch.world) and other(0, ch.world) == 0  # each entry refuses the other's plans
    rec = []
    for t in range(steps):
        gen = torch.Generator().manual_seed(2000 + t)
        for x in g16:
            x.copy_((torch.randn(x.shape, generator=gen) * float(2 ** t)).to(ch.dev))
        hyper = _lib.sgd_hyper([hp + (t == 0,)] * n)
        n0 = ch.stub.psgd_stub_calls()
        inner._table.fill(views)
        for tab, d in zip(f32 + b16, (P, B, scratch, w)):
            tab.fill(d.views)
        b16[1].fill(g16)
        if fused or not ok:
            call = lambda wd=wide: plan.aggregate_mixed_comm_sgd(  # noqa: E731
                b16[1].comp_addr(), inner._table.comp_addr(), b16[0].comp_addr(), f32[0].comp_addr(), f32[1].comp_addr(),
                hyper, codec.step_counter, codec._comm if comm else None, ch.stream, flat=inner._unc.plan,
                unc_bf16=b16[1].unc_addr(), unc_residual=inner._table.unc_addr(), unc_params_bf16=b16[0].unc_addr(),
                unc_masters=f32[0].unc_addr(), unc_bufs=f32[1].unc_addr(), wide=wd)
            if not ok:
                live = [residual, codec._ps_buffer, codec._qs_buffer, w.flat, P.flat, B.flat] + g16
                keep = [x.clone() for x in live]
                with pytest.raises(ValueError, match="no admitted update instance"):
                    call()
                torch.cuda.synchronize()
                assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(live, keep))
                assert ch.stub.psgd_stub_calls() == n0
                inner.close()
                return None
            with pytest.raises((ValueError, RuntimeError), match="serves rank"):  # the other entry refuses this plan
                call(not wide)
            call()
            codec.step_counter += 1
        else:
            hold = []  # the pointer arrays of this step's calls
            arr = lambda xs: hold.append(_lib.ptr_array(xs)) or ctypes.addressof(hold[-1])  # noqa: E731
            add.add_list(arr([x.data_ptr() for x in g16]), arr([x.data_ptr() for x in views]), True, ch.stream)
            if wide:
                avg = inner.aggregate(views)  # psgd_aggregate_comm: the fp32 slab and the flat slab
            else:
                plan.aggregate_comm_dst(inner._table.comp_addr(), f32[2].comp_addr(), codec.step_counter, codec._comm,
                                        ch.stream, flat=inner._unc.plan, unc=inner._table.unc_addr(), unc_dst=f32[2].unc_addr())
                codec.step_counter += 1
                avg = scratch.views
            _lib.sgd_update_mp(plan, *(arr([xs[i].data_ptr() for i in order]) for xs in (avg, P.views, B.views, w.views)),
                               [numel[i] for i in order], hyper, ch.stream)
        torch.cuda.synchronize()
        rec.append({"calls": ch.stub.psgd_stub_calls() - n0, "residual": _bits(residual).cpu(),
                    "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu(),
                    "canary": P.intact() and B.intact() and w.intact(), "g16_zero": all(not bool(_b16(x).any()) for x in g16),
                    "w": [_b16(x).cpu() for x in w.views], "p": [_bits(x).cpu() for x in P.views],
                    "buf": [_bits(x).cpu() for x in B.views]})
    assert mom or torch.equal(B.flat, b0), "the placeholder buf is neither read nor written without momentum"
    inner.close()
    return rec


def _entry(_, init, rank, iters):
    ch = _Child(init, 1)
    shapes = MODEL if rank > 32 else SHAPES
    try:
        for world in (1, 2):  # 1: shared terms, the fused call without a communicator; 2: two term sets
            ch.world = world
            for name in ("plain", "nesterov"):  # without momentum; momentum + weight decay + nesterov
                ref = _run(ch, shapes, rank, iters, HYPER[name], False)
                if (rank, iters) == (8, 2):  # refused like its twins, and touches nothing (checked in _run)
                    assert ref is None
                    continue
                assert ref is not None, (world, rank, iters, "the query must be 1")
                assert [r["calls"] for r in ref] == [iters + 1] * 3 and any(bool(r["residual"].any()) for r in ref)
                for shift in (0, 1):  # the vector form; w one element in: 2-byte stores
                    one = _run(ch, shapes, rank, iters, HYPER[name], True, shift, comm=world > 1)
                    for t, (x, y) in enumerate(zip(one, ref)):
                        ctx = (world, rank, iters, name, shift, t)
                        for k in ("p", "buf", "w"):
                            assert all(torch.equal(a, b) for a, b in zip(x[k], y[k])), (ctx, k)
                        for k in ("residual", "ps", "qs"):
                            assert torch.equal(x[k], y[k]), (ctx, k)
                        assert x["calls"] == (y["calls"] if world > 1 else 0), (ctx, "collective count")
                        assert x["canary"] and x["g16_zero"], ctx
                        assert not any(bool((a == W_CANARY).any()) for a in x["w"]), (ctx, "a bf16 weight was never stored")
    finally:
        ch.close()


@pytest.mark.parametrize("rank,iters", [(1, 1), (2, 2), (4, 3), (16, 2), (32, 2), (8, 2), (40, 1), (64, 2)])
def test_mixed_sgd_entries_equal_their_definitions_bitwise(rank, iters, tmp_path):
    """psgd_aggregate_mixed_comm_sgd (ranks 40 and 64: _wide) against the ADD + psgd_aggregate_comm_dst
    (psgd_aggregate_comm) + psgd_sgd_update_mp: raw bits of every master, buffer, bf16 weight, residual and P/Q
    buffer after each of 3 steps, the gradients all +0.0, the collective count, the canaries; world 1 and 2,
    w aligned and one element in, with and without momentum; (8, 2) refuses and touches nothing."""
    torch.multiprocessing.spawn(_entry, args=(_init(tmp_path), rank, iters), nprocs=1, join=True)


# ------------------------------------------------------------------ test 3: sgd_master_step
HP = HYPER["mom_wd"]


def _setup(rank, start=1, opt_kw=None, **agg_kw):
    from powersgd_amd import Config, Fp32ResidualPowerSGD

    gen = torch.Generator().manual_seed(3)
    masters = [torch.nn.Parameter(torch.randn(s, generator=gen).to("cuda:0")) for s in MODEL]
    model = [torch.nn.Parameter(p.detach().bfloat16()) for p in masters]
    opt = torch.optim.SGD(masters, **{**dict(lr=HP[0], momentum=HP[1], weight_decay=HP[3], foreach=False), **(opt_kw or {})})
    agg = Fp32ResidualPowerSGD(model, Config(rank, 0.5, 2, start), **agg_kw)
    for x in model:
        x.grad = torch.zeros_like(x)
    return masters, model, opt, agg


def _master_step(_, initfile, rank):
    from powersgd_amd import sgd_master_step, sgd_master_step_applies

    torch.cuda.set_device(0)
    torch.distributed.init_process_group("nccl", init_method=f"file://{initfile}", rank=0, world_size=1,
                                         device_id=torch.device("cuda:0"))
    try:
        (pa, wa, oa, ga), (pb, wb, ob, gb) = _setup(rank), _setup(rank)
        assert ga.inner._powersgd._plan.is_wide() == (rank > 32)
        seen = {}
        ob.register_step_pre_hook(lambda *_: seen.update(g=[p.grad.detach().clone() for p in pb]))
        for t in range(3):  # one warm-up step, then both parities
            before = [(y.data.clone(), ob.state[y]["momentum_buffer"].clone()) for y in pb] if t else None
            gen = torch.Generator().manual_seed(500 + t)
            for x, y in zip(wa, wb):
                x.grad = torch.randn(x.shape, generator=gen).to(x.device, x.dtype)
                y.grad = x.grad.clone()
            assert sgd_master_step_applies(oa, ga, wa) == (t >= 1), t
            sgd_master_step(oa, ga, wa)
            for p, a in zip(pb, gb.aggregate_fp32([y.grad for y in wb])):  # the unfused sequence, on the copy
                p.grad = a
            ob.step()
            for p, y in zip(pb, wb):
                p.grad = None
                y.data.copy_(p.data)
            torch.cuda.synchronize()
            assert torch.equal(_bits(ga.residual), _bits(gb.residual)), (t, "residual")
            for i, (x, y) in enumerate(zip(pa, pb)):
                bx, by = oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"]
                assert set(oa.state[x]) == set(ob.state[y]) and x.grad is None and not bool(_b16(wa[i].grad).any()), (t, i)
                assert torch.equal(_b16(wa[i].data), _b16(x.data.bfloat16())), (t, i, "model != bf16(master)")
                if t:
                    want_p, want_b, bound, bound_b = _ref64(HP, False, seen["g"][i].cpu(), *(s.cpu() for s in before[i]))
                    for got, ref, f64, bd, k in ((x.data, y.data, want_p, bound, "p"), (bx, by, want_b, bound_b, "buf")):
                        assert bool(((got - ref).cpu().double().abs() <= 2 * bd).all()), (t, i, k, "unfused")
                        assert bool(((got.cpu().double() - f64).abs() <= 2 * bd).all()), (t, i, k, "float64")
                x.data.copy_(y.data)  # identical state before the next step: bounds do not compound
                bx.copy_(by)
        # what keeps the unfused sequence (host-level checks on a compressing step)
        for opt_kw, agg_kw in ((None, dict(max_grad_norm=1.0)), (dict(nesterov=True), {}), (dict(maximize=True), {})):
            pc, wc, oc, gc = _setup(rank, start=0, opt_kw=opt_kw, **agg_kw)
            if opt_kw and "nesterov" in opt_kw:
                assert sgd_master_step_applies(oc, gc, wc)  # nesterov alone is served
                oc.param_groups[0]["dampening"] = 0.1
            assert not sgd_master_step_applies(oc, gc, wc), (opt_kw, agg_kw)
        pc, wc, _, gc = _setup(rank, start=0)
        assert not sgd_master_step_applies(torch.optim.Adagrad(pc, lr=0.1), gc, wc)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("rank", [4, 64])
def test_sgd_master_step_against_unfused_sequence(rank, tmp_path):
    """SGD with momentum and weight decay on fp32 masters of a bf16 model in a one-rank process group, two
    iterations, one warm-up step then both parities: masters and buffers within 2 x THE BOUND of the unfused
    sequence and of float64 on its averages, from the same state; model weights bitwise master.bfloat16(), the
    residual bitwise, the state dict torch's, gradients zero; and the options that keep the unfused sequence."""
    torch.multiprocessing.spawn(_master_step, args=(str(tmp_path / "init"), rank), nprocs=1, join=True)
