"""The fused AdamW step of a bf16 model with fp32 master weights (include/psgd.h: psgd_adam_update_mp,
psgd_aggregate_mixed_comm_adam; powersgd_amd/adam_master.py). THE BOUND is test_gpu_adam_step.py's,
derived in its docstring; the bf16 weights have no tolerance: w == bf16(stored fp32 p'), raw bits."""
import ctypes

import pytest
import torch

from test_gpu_adam_step import HYPER, _ref64, _within
from test_gpu_comm_dst import NUMEL, SHAPES, _bits, _Child, _Dst, _fresh, _init, _layout

pytestmark = pytest.mark.gpu
W_CANARY = 0x7FC1  # a bf16 quiet NaN with a payload


def _b16(x):
    return x.contiguous().view(torch.int16)


# ------------------------------------------------------------------ test 1: the element-wise kernel
LENGTHS = (1, 3, 4, 5, 4096, 4097)


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("name", ["adamw", "lerp_hi"])
def test_adam_update_mp_against_float64(name, t):
    """k_adam_update_mp alone, every case a tensor of ONE launch: p', m', v' within THE BOUND of float64,
    w bitwise bf16(p'), NaN canaries round every tensor intact, g unchanged. Offsets (0,0,0,0 | 0) and
    (1,1,1,1 | 1) take the vector form, every other case the element form."""
    from powersgd_amd import _lib

    dev = torch.device("cuda:0")
    cases = [(n, og, op, om, ov, ow) for n in LENGTHS for og in (0, 1) for op in (0, 1) for om in (0, 1)
             for ov in (0, 1) for ow in (0, 1, 2)]
    slot = 8 + max(LENGTHS) + 8 + (-(16 + max(LENGTHS))) % 4  # canaries either side, a multiple of 4 elements
    gen = torch.Generator().manual_seed(11)
    flat = {k: torch.full((len(cases) * slot,), float("nan")) for k in "gpmv"}
    lo = {k: [i * slot + 8 + c[1 + j] for i, c in enumerate(cases)] for j, k in enumerate("gpmvw")}
    for i, c in enumerate(cases):
        for k in "gpmv":
            x = torch.randn(c[0], generator=gen)
            flat[k][lo[k][i]:lo[k][i] + c[0]] = x * x if k == "v" else x
    devb = {k: flat[k].to(dev) for k in "gpmv"}
    devb["w"] = torch.full((len(cases) * slot,), W_CANARY, dtype=torch.int16, device=dev)
    assert all(devb[k].data_ptr() % 16 == 0 for k in "gpmvw")
    ptrs = {k: _lib.ptr_array([devb[k].data_ptr() + devb[k].element_size() * o for o in lo[k]]) for k in "gpmvw"}
    hyper = _lib.adam_hyper([HYPER[name] + (float(t),)] * len(cases))
    _lib.adam_update_mp(None, *(ctypes.addressof(ptrs[k]) for k in "gpmvw"), [c[0] for c in cases], hyper,
                        torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out = {k: devb[k].cpu() for k in "gpmvw"}
    assert torch.equal(_bits(out["g"]), _bits(flat["g"])), "g is read only"
    inside = {k: torch.zeros(len(cases) * slot, dtype=torch.bool) for k in "pmvw"}
    worst = 0.0
    for i, c in enumerate(cases):
        cut = lambda src: [src[k][lo[k][i]:lo[k][i] + c[0]] for k in "gpmv"]  # noqa: E731
        want, bound = _ref64(hyper[0], *cut(flat))
        worst = max(worst, _within(cut(out)[1:], want, bound, c))
        w = out["w"][lo["w"][i]:lo["w"][i] + c[0]]
        assert torch.equal(w, _b16(cut(out)[1].bfloat16())), (c, "w != bf16(p')")
        for k in "pmvw":
            inside[k][lo[k][i]:lo[k][i] + c[0]] = True
    for k in "pmv":
        assert torch.equal(_bits(out[k])[~inside[k]], _bits(flat[k])[~inside[k]]), (k, "canary")
    assert bool((out["w"][~inside["w"]] == W_CANARY).all()), "w canary"
    print(f"adam_update_mp {name} t={t}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------ test 2: the entry against its definition
class _W:
    """The bf16 model tensors in one bucket-like buffer, canary everywhere: every view 8-byte aligned
    (`shift` 0) or one element in (2-byte aligned only)."""

    def __init__(self, shift, dev):
        offs, total = _layout(0)
        self.flat = torch.full((total,), W_CANARY, dtype=torch.int16, device=dev)
        self.views = [self.flat[o + shift:o + shift + n].view(torch.bfloat16).view(s) for o, n, s in zip(offs, NUMEL, SHAPES)]
        assert all(v.data_ptr() % 8 == 2 * shift for v in self.views)
        self.outside = torch.ones(total, dtype=torch.bool, device=dev)
        for o, n in zip(offs, NUMEL):
            self.outside[o + shift:o + shift + n] = False

    def canary_intact(self):
        return bool((self.flat[self.outside] == W_CANARY).all())


def _run(ch, rank, iters, fused, shift=0, comm=True, steps=3):
    """`steps` steps of psgd_aggregate_mixed_comm_adam (`fused`) or of its defining sequence: the ADD,
    psgd_aggregate_comm_dst into scratch, psgd_adam_update_mp. A plan that is not admitted: asserts that
    the call refuses and touches nothing, returns None."""
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import _psgd_host

    residual, views, inner = ch.codec(rank, iters)
    codec, plan = inner._powersgd, inner._powersgd._plan
    pmv = [_Dst("aligned", ch.dev) for _ in range(3)]
    gen = torch.Generator().manual_seed(77)
    for x in pmv[0].views:
        x.copy_(torch.randn(x.shape, generator=gen))
    for d in pmv[1:]:
        for x in d.views:
            x.zero_()
    w, scratch = _W(shift, ch.dev), _Dst("aligned", ch.dev)
    g16 = [torch.zeros(s, dtype=torch.bfloat16, device=ch.dev) for s in SHAPES]
    mask = inner.is_compressed_mask
    n = len(SHAPES)
    f32 = [_psgd_host.PtrTable([list(s) for s in SHAPES], mask, _lib.PSGD_F32, 0) for _ in range(4)]
    b16 = [_psgd_host.PtrTable([list(s) for s in SHAPES], mask, _lib.PSGD_BF16, 0) for _ in range(2)]
    add = _lib.Runs([0] * n, list(range(n)), [0] * n, NUMEL, n, _lib.PSGD_F32, _lib.PSGD_BF16, source=list(range(n)), nsources=n)
    ws = torch.empty(add.workspace_bytes(), dtype=torch.uint8, device=ch.dev)
    add.bind(0, ws.data_ptr())
    order = [i for i, c in enumerate(mask) if c] + [i for i, c in enumerate(mask) if not c]
    ok = plan.mixed_adam_ok(0, ch.world)
    assert ok == plan.mixed_adam_ok(1, ch.world)
    rec = []
    for t in range(steps):
        for x, g in zip(g16, _fresh(t)):
            x.copy_(g.to(ch.dev))
        hyper = _lib.adam_hyper([HYPER["adamw"] + (float(t + 1),)] * n)
        n0 = ch.stub.psgd_stub_calls()
        inner._table.fill(views)
        for tab, d in zip(f32 + b16, pmv + [scratch, w]):
            tab.fill(d.views)
        b16[1].fill(g16)
        if fused or not ok:
            call = lambda: plan.aggregate_mixed_comm_adam(  # noqa: E731
                b16[1].comp_addr(), inner._table.comp_addr(), b16[0].comp_addr(), *(x.comp_addr() for x in f32[:3]), hyper,
                codec.step_counter, codec._comm if comm else None, ch.stream, flat=inner._unc.plan,
                unc_bf16=b16[1].unc_addr(), unc_residual=inner._table.unc_addr(), unc_params_bf16=b16[0].unc_addr(),
                unc_masters=f32[0].unc_addr(), unc_ms=f32[1].unc_addr(), unc_vs=f32[2].unc_addr())
            if not ok:
                live = [residual, codec._ps_buffer, codec._qs_buffer, w.flat] + [d.flat for d in pmv] + g16
                keep = [x.clone() for x in live]
                with pytest.raises(ValueError, match="no admitted update instance"):
                    call()
                torch.cuda.synchronize()
                assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(live, keep))
                assert ch.stub.psgd_stub_calls() == n0
                inner.close()
                return None
            call()
        else:
            hold = []  # the pointer arrays of this step's three calls
            arr = lambda xs: hold.append(_lib.ptr_array(xs)) or ctypes.addressof(hold[-1])  # noqa: E731
            add.add_list(arr([x.data_ptr() for x in g16]), arr([x.data_ptr() for x in views]), True, ch.stream)
            plan.aggregate_comm_dst(inner._table.comp_addr(), f32[3].comp_addr(), codec.step_counter, codec._comm, ch.stream,
                                    flat=inner._unc.plan, unc=inner._table.unc_addr(), unc_dst=f32[3].unc_addr())
            _lib.adam_update_mp(plan, *(arr([d.views[i].data_ptr() for i in order]) for d in [scratch] + pmv + [w]),
                                [NUMEL[i] for i in order], hyper, ch.stream)
        codec.step_counter += 1
        torch.cuda.synchronize()
        rec.append({"calls": ch.stub.psgd_stub_calls() - n0, "residual": _bits(residual).cpu(),
                    "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu(),
                    "canary": all(d.canary_intact() for d in pmv + [w]),
                    "g16_zero": all(not bool(_b16(x).any()) for x in g16),
                    "w": [_b16(x).cpu() for x in w.views], **{k: [_bits(x).cpu() for x in d.views] for k, d in zip("pmv", pmv)}})
    inner.close()
    return rec


def _entry(_, init, rank, iters):
    ch = _Child(init, 1)
    try:
        for world in (1, 2):  # 1: shared terms, the fused call without a communicator; 2: two term sets
            ch.world = world
            ref = _run(ch, rank, iters, False)
            if (rank, iters) == (8, 2):  # refused like its twins, and touches nothing (checked in _run)
                assert ref is None
                continue
            assert ref is not None, (world, rank, iters, "psgd_plan_mixed_adam_ok must be 1")
            assert [r["calls"] for r in ref] == [iters + 1] * 3 and any(bool(r["residual"].any()) for r in ref)
            for shift in (0, 1):  # the vector form; w one element in: the element form
                one = _run(ch, rank, iters, True, shift, comm=world > 1)
                for t, (x, y) in enumerate(zip(one, ref)):
                    ctx = (world, rank, iters, shift, t)
                    for k in "pmvw":
                        assert all(torch.equal(a, b) for a, b in zip(x[k], y[k])), (ctx, k)
                    for k in ("residual", "ps", "qs"):
                        assert torch.equal(x[k], y[k]), (ctx, k)
                    assert x["calls"] == (y["calls"] if world > 1 else 0), (ctx, "collective count")
                    assert x["canary"] and x["g16_zero"], ctx
                    assert not any(bool((a == W_CANARY).any()) for a in x["w"]), (ctx, "a bf16 weight was never stored")
    finally:
        ch.close()


@pytest.mark.parametrize("rank,iters", [(1, 1), (1, 2), (2, 2), (4, 3), (8, 1), (16, 2), (32, 2), (8, 2)])
def test_mixed_adam_entry_equals_its_definition_bitwise(rank, iters, tmp_path):
    """psgd_aggregate_mixed_comm_adam against the ADD + psgd_aggregate_comm_dst + psgd_adam_update_mp: raw bits
    of every master, moment, bf16 weight, residual and P/Q buffer after each of 3 steps, the gradients
    all +0.0, the collective count, the canaries; (8, 2) refuses with PSGD_ERR_VALUE and touches nothing."""
    torch.multiprocessing.spawn(_entry, args=(_init(tmp_path), rank, iters), nprocs=1, join=True)


# ------------------------------------------------------------------ test 3: adam_master_step
MODEL = [(32, 16, 3, 3), (64, 32), (48, 24), (32,), (3, 100)]
KEYS = ("exp_avg", "exp_avg_sq")


def _setup(start=1, **agg_kw):
    from powersgd_amd import Config, Fp32ResidualPowerSGD

    gen = torch.Generator().manual_seed(3)
    masters = [torch.nn.Parameter(torch.randn(s, generator=gen).to("cuda:0")) for s in MODEL]
    model = [torch.nn.Parameter(p.detach().bfloat16()) for p in masters]
    opt = torch.optim.AdamW(masters, lr=1e-3, weight_decay=1e-2, foreach=False)
    agg = Fp32ResidualPowerSGD(model, Config(rank=2, min_compression_rate=2, num_iters_per_step=2,
                                             start_compressing_after_num_steps=start), **agg_kw)
    return masters, model, opt, agg


def _master_step(_, initfile):
    from powersgd_amd import _lib, adam_master_step, adam_master_step_applies

    torch.cuda.set_device(0)
    torch.distributed.init_process_group("nccl", init_method=f"file://{initfile}", rank=0, world_size=1,
                                         device_id=torch.device("cuda:0"))
    try:
        pa, wa, oa, ga = _setup()
        pb, wb, ob, gb = _setup()
        seen = {}
        ob.register_step_pre_hook(lambda *_: seen.update(g=[p.grad.detach().clone() for p in pb]))
        for t in range(4):  # one warm-up step, then three compressing ones
            before = [[y.data.clone()] + [ob.state[y][k].clone() for k in KEYS] for y in pb] if t else None
            gen = torch.Generator().manual_seed(500 + t)
            for x, y in zip(wa, wb):
                x.grad = torch.randn(x.shape, generator=gen).to(x.device, x.dtype)
                y.grad = x.grad.clone()
            assert adam_master_step_applies(oa, ga, wa) == (t >= 1), t
            adam_master_step(oa, ga, wa)
            # the unfused sequence, on the copy
            for p, a in zip(pb, gb.aggregate_fp32([y.grad for y in wb])):
                p.grad = a
            ob.step()
            for p, y in zip(pb, wb):
                p.grad = None
                y.data.copy_(p.data)
            torch.cuda.synchronize()
            assert torch.equal(_bits(ga.residual), _bits(gb.residual)), (t, "residual")
            for i, (x, y) in enumerate(zip(pa, pb)):
                sx, sy = oa.state[x], ob.state[y]
                assert sx["step"].device.type == "cpu" and float(sx["step"]) == float(sy["step"]) == t + 1, (t, i)
                assert x.grad is None and not bool(_b16(wa[i].grad).any()) and not bool(_b16(wb[i].grad).any()), (t, i)
                assert torch.equal(_b16(wa[i].data), _b16(x.data.bfloat16())), (t, i, "model != bf16(master)")
                if t:
                    h = _lib.adam_hyper([(1e-3, 0.9, 0.999, 1e-8, 1e-2, True, float(t + 1))])[0]
                    _, bound = _ref64(h, seen["g"][i].cpu(), *(b.cpu() for b in before[i]))
                    got = [x.data.cpu()] + [sx[k].cpu() for k in KEYS]
                    want = [y.data.cpu().double()] + [sy[k].cpu().double() for k in KEYS]
                    _within(got, want, bound, (t, i), scale=2.0)
                x.data.copy_(y.data)  # identical state before the next step: bounds do not compound
                for k in KEYS:
                    sx[k].copy_(sy[k])
        # clipping keeps the unfused sequence (a host-level check)
        pc, wc, oc, gc = _setup(start=0, max_grad_norm=1.0)
        for x in wc:
            x.grad = torch.zeros_like(x)
        assert not adam_master_step_applies(oc, gc, wc)
    finally:
        torch.distributed.destroy_process_group()


def test_adam_master_step_against_unfused_sequence(tmp_path):
    """AdamW with weight decay on fp32 masters of a bf16 model in a one-rank process group, rank 2, two
    iterations, one warm-up step then both parities: masters and moments within 2 x THE BOUND of the unfused
    sequence from the same state, model weights bitwise master.bfloat16(), state["step"] equal, gradients zero."""
    torch.multiprocessing.spawn(_master_step, args=(str(tmp_path / "init"),), nprocs=1, join=True)
