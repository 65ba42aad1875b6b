"""``Fp32ResidualPowerSGD(..., fused=True)`` at ranks 33-128 (psgd_aggregate_mixed_wide[_comm]: the
final pass k_wide_apply_mix stages the factor blocks in LDS and stores the bf16 averages) against
the three-stage flow of the same build (``fused=False``: run-table ADD, the fp32 wide codec,
run-table GATHER), bit for bit, and against a float64 restatement of the step on the CPU.

The shapes (fp32 residual views back to back, in this order): (130, 321) odd m: 2-byte output
stores and scalar residual access, three row blocks, two column tiles; (96, 260) twice: a
two-matrix group; (100, 13): capped at r = 13 inside a wide plan; (65, 512): two full column tiles,
one row past a block; (257, 260): a residual view that is 8-byte aligned only; (40,): the flat
tail. Ranks 33 (bucket 64, r % 4 != 0), 64, 100 (bucket 128, r < R) and 128.

In that order every view after (130, 321) (41730 elements, 2 mod 4) is 8-byte aligned only and
every later bf16 output offset 4-byte aligned only, so the kernel takes its scalar residual access
and its 2-byte output stores throughout. The second order, "aligned", puts the matrices with
m % 4 = 0 first: their residual views are 16-byte aligned and their output offsets 8-byte aligned,
which is the 16-byte residual load / store and the 8-byte packed output store that dense
workloads take. test_alignment_classes pins both from the pointers.

Reference bounds (step 0, I = 2): the residual within TOL_STEP = 1e-5 of the input's norm, the
metric and bound of tests/test_gpu_wide_rank.py; each bf16 average within 2^-8 |ref| (one bf16
rounding: half an ulp of 2^-7) + 1e-5 max|input| (the fp32 step's own error, that same bound).
Observed worst values: DESIGN.md section 5."""
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
SHAPES = [(130, 321), (96, 260), (96, 260), (100, 13), (65, 512), (257, 260), (40,)]
ORDERS = {"issue": SHAPES,
          "aligned": [(96, 260), (96, 260), (65, 512), (257, 260), (100, 13), (130, 321), (40,)]}
STEPS = 3
TOL_STEP = 1e-5


def _mcr(iters: int) -> float:
    # numel / (0.5 I min(rank, min(shape)) sum(shape)): the smallest compressed one is (130, 321) at
    # rank 128, 1.446 / I; (40,) is at most 2 / (33 I)
    return 1.4 / iters


def _fresh(t: int, order: str = "issue"):
    """Seeded bf16 gradients of step t, growing each step; a few -0.0 among them."""
    gen = torch.Generator().manual_seed(2000 + t)
    out = []
    for s in ORDERS[order]:
        g = (torch.randn(s, generator=gen) * float(2 ** t)).to(BF16)
        g.view(-1)[::7] = -0.0
        out.append(g)
    return out


def _place(fresh, odd: bool):
    """Separate tensors, or views at odd element offsets of one bf16 buffer (2-byte aligned only)."""
    if not odd:
        return [g.to(DEV) for g in fresh]
    flat = torch.zeros(sum(g.numel() + 2 for g in fresh) + 1, dtype=BF16, device=DEV)
    views, off = [], 1
    for g in fresh:
        v = flat[off:off + g.numel()].view(g.shape)
        assert v.data_ptr() % 4 == 2
        v.copy_(g)
        views.append(v)
        off += g.numel() + (2 if g.numel() % 2 == 0 else 1)
    return views


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


def _aggregator(rank: int, iters: int, fused: bool, comm=None, order: str = "issue"):
    from powersgd_amd import Config, Fp32ResidualPowerSGD

    shapes = ORDERS[order]
    agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=BF16, device=DEV) for s in shapes],
                               Config(rank, _mcr(iters), iters, 0), fused=fused)
    assert agg.is_compressed_mask == [len(s) > 1 for s in shapes]
    assert agg.inner._powersgd._plan.is_wide()
    if comm is not None:
        agg.inner._powersgd._comm = comm
    return agg


def _flow(rank: int, iters: int, odd: bool, fused: bool, comm=None, order: str = "issue"):
    """STEPS steps of one aggregator; per step the raw bits of everything observable."""
    agg = _aggregator(rank, iters, fused, comm, order)
    rec = []
    for t in range(STEPS):
        grads = _place(_fresh(t, order), odd)
        folds = agg.fused_folds()
        out = agg.aggregate(grads)
        torch.cuda.synchronize()
        codec = agg.inner._powersgd
        rec.append({"folds": folds, "out": [_bits(o).cpu() for o in out], "residual": _bits(agg.residual).cpu(),
                    "ps": _bits(codec._ps_buffer).cpu(), "qs": _bits(codec._qs_buffer).cpu(),
                    "grads_zero": all(not bool(_bits(g).any()) for g in grads)})
    agg.close()
    return rec


@functools.lru_cache(maxsize=None)
def _unfused(rank: int, iters: int, odd: bool, order: str = "issue"):
    return _flow(rank, iters, odd, False, order=order)  # the reference: computed once, never modified


def _same(a, b, ctx):
    for t, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x["out"], y["out"])):
            assert torch.equal(p, q), (ctx, t, i, "output")
        for k in ("residual", "ps", "qs"):
            assert torch.equal(x[k], y[k]), (ctx, t, k)
        assert x["grads_zero"] and y["grads_zero"], (ctx, t, "every gradient element is +0.0")


def _compare(rank, iters, odd, flow=_flow, ref=None, order="issue"):
    ctx = (rank, iters, odd, order)
    ref = ref or _unfused(rank, iters, odd, order)
    assert [r["folds"] for r in ref] == [(0, 0)] * STEPS
    one = flow(rank, iters, odd, True, order=order)
    assert [r["folds"] for r in one] == [(0, 1)] * STEPS, (ctx, [r["folds"] for r in one])
    _same(one, ref, ctx)
    _same(flow(rank, iters, odd, True, order=order), one, (ctx, "second fused run"))
    assert any(bool(r["residual"].any()) for r in one)


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("rank", [33, 64, 100, 128])
def test_fused_equals_three_stage_flow_bitwise(rank, iters):
    _compare(rank, iters, False)


def test_fused_equals_three_stage_flow_bitwise_odd_offset_views():
    _compare(64, 2, True)


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("rank", [64, 100, 128])
def test_fused_equals_three_stage_flow_bitwise_aligned_order(rank, iters):
    """The 16-byte residual access and the 8-byte output store (world size 1: the shared form)."""
    _compare(rank, iters, False, order="aligned")


@pytest.mark.parametrize("rank", [64, 128])
def test_alignment_classes(rank):
    """What k_wide_apply_mix tests per matrix, from the residual views' pointers, the plan's output
    offsets (bf16 elements) and the shapes: gvec (m % 4 = 0, view 16-byte aligned) and ovec
    (m % 4 = 0, output address 8-byte aligned; the slab's base is 16-byte aligned)."""
    want = {"issue": {(130, 321): (False, False), (96, 260): (False, False), (100, 13): (False, False),
                      (65, 512): (False, False), (257, 260): (False, False)},
            "aligned": {(96, 260): (True, True), (65, 512): (True, True), (257, 260): (True, True),
                        (100, 13): (False, False), (130, 321): (False, False)}}
    for order, shapes in ORDERS.items():
        agg = _aggregator(rank, 2, True, order=order)
        comp = [i for i, c in enumerate(agg.is_compressed_mask) if c]
        offs = dict(zip(comp, agg.inner._powersgd._plan.output_offsets()))
        for i in comp:
            m = shapes[i][1]
            got = (m % 4 == 0 and agg.views[i].data_ptr() % 16 == 0, m % 4 == 0 and (offs[i] * 2) % 8 == 0)
            assert got == want[order][shapes[i]], (order, shapes[i], got)
        if order == "issue":  # 8-byte aligned only, as every view after the first there
            assert agg.views[shapes.index((257, 260))].data_ptr() % 16 == 8
        agg.close()


def test_direct_call_equals_the_sequence_and_rank_32_is_refused():
    from powersgd_amd import _lib
    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    shapes = [s for s in SHAPES if len(s) > 1]
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def run(rank: int, direct: bool):
        codec = BasicPowerSGD([torch.zeros(s, device=DEV) for s in shapes], BasicConfig(rank, 2))
        assert codec._plan.mixed_wide_ok(1) == (1 if rank > 32 else 0)
        gen = torch.Generator().manual_seed(5)
        grads = [torch.randn(s, generator=gen).to(BF16).to(DEV) for s in shapes]
        resid = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
        if direct:
            out = torch.full((sum(g.numel() for g in grads),), 3.0, dtype=BF16, device=DEV)
            gp = _lib.ptr_array([g.data_ptr() for g in grads])
            rp = _lib.ptr_array([r.data_ptr() for r in resid])
            codec._plan.aggregate_mixed_wide(ctypes.addressof(gp), ctypes.addressof(rp), out.data_ptr(), 0, stream)
        else:
            for r, g in zip(resid, grads):
                r += g.float()
                g.zero_()
            out = torch.cat([o.reshape(-1) for o in codec.aggregate(resid)]).to(BF16)
        torch.cuda.synchronize()
        return [_bits(x).cpu() for x in [out] + grads + resid + [codec._ps_buffer, codec._qs_buffer]]

    for x, y in zip(run(64, True), run(64, False)):
        assert torch.equal(x, y)
    codec = BasicPowerSGD([torch.zeros(s, device=DEV) for s in shapes], BasicConfig(32, 2))
    assert codec._plan.mixed_wide_ok(1) == 0
    state = [torch.randn(s).to(BF16).to(DEV) for s in shapes] + [torch.randn(s, device=DEV) for s in shapes]
    out = torch.full((sum(torch.Size(s).numel() for s in shapes),), 3.0, dtype=BF16, device=DEV)
    keep = [_bits(x).clone() for x in state + [out, codec._ps_buffer, codec._qs_buffer]]
    gp = _lib.ptr_array([g.data_ptr() for g in state[:len(shapes)]])
    rp = _lib.ptr_array([r.data_ptr() for r in state[len(shapes):]])
    with pytest.raises(ValueError, match="psgd_aggregate_mixed_wide serves ranks 33-128"):
        codec._plan.aggregate_mixed_wide(ctypes.addressof(gp), ctypes.addressof(rp), out.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    for a, b in zip(state + [out, codec._ps_buffer, codec._qs_buffer], keep):
        assert torch.equal(_bits(a), b)


def _comm_child(_, init):
    """World size 2 on one GPU through the stand-in collective library (tests/test_gpu_mixed_comm.py)."""
    from powersgd_amd import _lib

    os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
    os.environ["PSGD_TESTING"] = "1"
    torch.cuda.set_device(DEV)
    torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
    try:
        def flow(rank, iters, odd, fused, order="issue"):
            return _flow(rank, iters, odd, fused, _lib.Comm(2, 0, _lib.comm_unique_id(), 0), order)

        # the two-term-set form: the issue's order (scalar access), then the aligned order (16-byte
        # residual access, 8-byte output stores) at both rank buckets
        for rank, order in ((64, "issue"), (64, "aligned"), (128, "aligned")):
            _compare(rank, 2, False, flow, flow(rank, 2, False, False, order), order)
    finally:
        torch.distributed.destroy_process_group()


def test_comm_entry_equals_its_three_stages_bitwise_world_2(tmp_path):
    torch.multiprocessing.spawn(_comm_child, args=(f"file://{tmp_path}/store",), nprocs=1, join=True)


@pytest.mark.parametrize("rank", [33, 128])
def test_step0_against_float64(rank):
    """Step 0, I = 2, from the codec's own initial P / Q, restated in float64: P0 = qr(P), Q0 = G^T P0,
    Q1 = qr(Q0), P1 = (G - P0 Q0^T) Q1, output = P0 Q0^T + P1 Q1^T, residual = G - output."""
    agg = _aggregator(rank, 2, True)
    codec = agg.inner._powersgd
    p0, q0 = codec._ps_buffer.double().cpu(), codec._qs_buffer.double().cpu()
    fresh = _fresh(0)
    out = agg.aggregate(_place(fresh, False))
    torch.cuda.synchronize()
    comp = [i for i, s in enumerate(SHAPES) if len(s) > 1]
    poff = qoff = 0
    worst_res = worst_out = 0.0
    for n, m, r, c in codec._plan.groups():
        for i in [i for i in comp if SHAPES[i] == (n, m)]:
            G = fresh[i].double()
            P = p0[poff:poff + n * r].view(n, r)
            poff, qoff = poff + n * r, qoff + m * r
            P0 = torch.linalg.qr(P).Q
            Q0 = G.t() @ P0
            Q1 = torch.linalg.qr(Q0).Q
            P1 = (G - P0 @ Q0.t()) @ Q1
            ref = P0 @ Q0.t() + P1 @ Q1.t()
            res_err = float((agg.views[i].double().cpu() - (G - ref)).norm() / G.norm())
            bound = 2.0 ** -8 * ref.abs() + TOL_STEP * float(G.abs().max())
            out_err = float(((out[i].double().cpu() - ref).abs() / bound).max())
            print(f"rank {rank} tensor {i} {SHAPES[i]}: residual {res_err:.3e}, output error / bound {out_err:.3f}")
            worst_res, worst_out = max(worst_res, res_err), max(worst_out, out_err)
    print(f"rank {rank}: worst residual {worst_res:.3e}, worst output error / bound {worst_out:.3f}")
    assert poff == p0.numel() and qoff == q0.numel()
    assert worst_res <= TOL_STEP and worst_out <= 1.0
    agg.close()
