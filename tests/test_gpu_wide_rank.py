"""Effective ranks 33-128 (the wide-rank path, psgd_wide.hip) against the CPU oracle.

Shape rule: every power iteration deflates r dimensions, so a factor left in the state is
rank-deficient once iters * r > min(n, m) (or r == min(n, m) with iters >= 2); its QR completion
is then decided by rounding and the reference diverges from itself at the next step. Free-running
comparisons therefore use sets A / B (iters * r <= min(n, m) everywhere); set N (narrow, masked
and rank-1 matrices inside a wide plan) gets the step-0 comparison and the error-feedback
identity, which stays meaningful where the oracle is chaotic.

Tolerances are the project's: per tensor ||ours - oracle||_F <= TOL * ||input||_F with TOL_STEP =
1e-5 from an identical state, TOL_FREE = 1e-4 free-running, TOL_BF16 = 4e-3 for bf16 gradients
(oracle on the bf16-rounded inputs). DESIGN.md section 5 quotes the worst observed errors."""
import pytest
import torch

from parity_log import check
from oracle import powersgd_oracle as O
from powersgd_amd import Config, PowerSGD, _lib
from powersgd_amd.reducers import RankKReducer
from powersgd_amd.workloads import hash_tensors

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-5
TOL_FREE = 1e-4
TOL_BF16 = 4e-3
DEV = torch.device("cuda:0")

SHAPES_A = [(300, 200), (200, 1000), (1000, 196), (256, 24, 3, 3), (197, 203), (300, 200), (40,)]
SHAPES_B = [(320, 300), (289, 1000), (1000, 288), (288, 32, 3, 3), (291, 293), (320, 300), (40,)]
SHAPES_N = [(300, 200), (64, 1000), (1000, 48), (129, 67), (77, 130), (1000, 16), (200, 1), (128, 8, 3, 3)]
SETS = {"A": SHAPES_A, "B": SHAPES_B, "N": SHAPES_N}


def _rel(a, b, scale) -> float:
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(float(scale.double().norm()), 1e-30)


def _pair(shapes, rank, iters, dtype=torch.float32):
    """GPU aggregator and oracle from the same initial P / Q."""
    psgd = PowerSGD([torch.zeros(s, device=DEV, dtype=dtype) for s in shapes], Config(rank, 0.1, iters, 0))
    ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 0.1, iters, 0)
    ora.codec.p_flat.copy_(psgd._powersgd._ps_buffer.cpu())
    ora.codec.q_flat.copy_(psgd._powersgd._qs_buffer.cpu())
    return psgd, ora


def _free_run(shapes, rank, iters, steps, tols, dtype=torch.float32, seed=60):
    psgd, ora = _pair(shapes, rank, iters, dtype)
    assert psgd._powersgd._plan.is_wide()
    res_d = [torch.zeros(s, device=DEV, dtype=dtype) for s in shapes]
    for t in range(steps):
        new = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=seed + t)]
        gd = [(r + x.to(DEV)).to(dtype) for r, x in zip(res_d, new)]
        gc = [g.float().cpu() for g in gd]  # the oracle sees exactly the GPU inputs
        scale = [g.clone() for g in gc]
        od = psgd.aggregate(gd)
        oc = O.policy_step(ora, gc)
        torch.cuda.synchronize()
        for i, g in enumerate(scale):
            eo, er = _rel(od[i].float(), oc[i], g), _rel(gd[i].float(), gc[i], g)
            print(f"rank {rank} iters {iters} step {t} tensor {i}: out {eo:.3e} res {er:.3e}")
            check(eo, tols[t], rank, iters, t, i, "out")
            check(er, tols[t], rank, iters, t, i, "res")
        res_d = gd
    return psgd, ora


@pytest.mark.parametrize("name,rank,iters", [("A", 33, 2), ("A", 48, 3), ("A", 64, 1), ("A", 64, 2), ("A", 64, 3),
                                             ("B", 96, 2), ("B", 96, 3), ("B", 128, 1), ("B", 128, 2)])
def test_free_running_vs_oracle(name, rank, iters):
    """Two steps with error feedback; iters = 1 covers an even step followed by an odd one."""
    _free_run(SETS[name], rank, iters, 2, (TOL_STEP, TOL_FREE))


@pytest.mark.parametrize("rank,iters", [(64, 2), (128, 2), (40, 3)])
def test_step0_narrow_and_masked_matrices(rank, iters):
    """Set N from identical state: effective ranks 64/128, 64, 48, 64/67, 64/77, 16, 1 (joint group
    norm) and 64/72; rank 40 is a bucket of 64 with every matrix masked."""
    _free_run(SHAPES_N, rank, iters, 1, (TOL_STEP,))


def test_error_feedback_identity_three_steps():
    shapes, rank, iters = SHAPES_N, 64, 2
    psgd = PowerSGD([torch.zeros(s, device=DEV) for s in shapes], Config(rank, 0.1, iters, 0))
    res = [torch.zeros(s, device=DEV) for s in shapes]
    for t in range(3):
        new = [torch.from_numpy(f).to(DEV) for f in hash_tensors(shapes, seed=160 + t)]
        gd = [r + x for r, x in zip(res, new)]
        orig = [g.clone() for g in gd]
        od = psgd.aggregate(gd)
        torch.cuda.synchronize()
        for i, g in enumerate(orig):
            assert bool(torch.isfinite(od[i]).all()) and bool(torch.isfinite(gd[i]).all())
            check(_rel(od[i] + gd[i], g, g), 1e-6, t, i, "ef-identity")
        assert bool(torch.isfinite(psgd._powersgd._ps_buffer).all())
        assert bool(torch.isfinite(psgd._powersgd._qs_buffer).all())
        res = gd


def _panels(flat, groups, side):
    """Per matrix [k, r] panels of a P (side 0) or Q (side 1) state buffer."""
    out, off = [], 0
    for n, m, r, c in groups:
        k = n if side == 0 else m
        blk = flat[off:off + c * k * r].view(c, k, r)
        out += [blk[b] for b in range(c)]
        off += c * k * r
    return out


@pytest.mark.parametrize("name,rank", [("A", 64), ("B", 128)])
def test_orthonormal_in_factor(name, rank):
    """After an iters = 1 step the state P is the in-factor the step orthonormalised: X^T X = I to
    1e-5, and at step 0 it is the oracle's factor including LAPACK's column signs."""
    shapes = SETS[name]
    psgd, ora = _pair(shapes, rank, 1)
    gd = [torch.from_numpy(f).to(DEV) for f in hash_tensors(shapes, seed=5)]
    gc = [g.cpu() for g in gd]
    psgd.aggregate(gd)
    O.policy_step(ora, gc)
    torch.cuda.synchronize()
    groups = psgd._powersgd._plan.groups()
    ours = _panels(psgd._powersgd._ps_buffer.cpu(), groups, 0)
    want = _panels(ora.codec.p_flat, groups, 0)
    for i, (x, w) in enumerate(zip(ours, want)):
        gram = x.double().t() @ x.double()
        dev = float((gram - torch.eye(x.shape[1], dtype=torch.float64)).abs().max())
        col = float((x.double() - w.double()).norm(dim=0).max())
        print(f"panel {i} {tuple(x.shape)}: |X^T X - I|max {dev:.3e}, worst column vs oracle {col:.3e}")
        check(dev, 1e-5, name, rank, i, "orthonormal")
        check(col, 1e-4, name, rank, i, "column-vs-oracle")


def test_zero_gradients():
    """Outputs and residuals exactly zero; the state is finite and the oracle's: the zero factor
    orthonormalises to the leading identity columns, as torch.linalg.qr gives."""
    shapes = SHAPES_A
    psgd, ora = _pair(shapes, 64, 2)
    gd = [torch.zeros(s, device=DEV) for s in shapes]
    od = psgd.aggregate(gd)
    O.policy_step(ora, [torch.zeros(s) for s in shapes])
    torch.cuda.synchronize()
    for o, g in zip(od, gd):
        assert not bool(o.any()) and not bool(g.any())
    for ours, want in ((psgd._powersgd._ps_buffer, ora.codec.p_flat), (psgd._powersgd._qs_buffer, ora.codec.q_flat)):
        assert bool(torch.isfinite(ours).all())
        assert float((ours.cpu() - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("name,rank", [("A", 64), ("B", 128)])
def test_bf16_gradients(name, rank):
    _free_run(SETS[name], rank, 2, 2, (TOL_BF16, TOL_BF16), dtype=torch.bfloat16)


@pytest.mark.parametrize("name,rank", [("A", 64), ("B", 128)])
def test_rerun_is_bitwise_identical(name, rank):
    shapes = SETS[name]
    psgd = PowerSGD([torch.zeros(s, device=DEV) for s in shapes], Config(rank, 0.1, 2, 0))
    p0, q0 = psgd._powersgd._ps_buffer.clone(), psgd._powersgd._qs_buffer.clone()
    grads = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=77)]
    runs = []
    for _ in range(2):
        psgd._powersgd._ps_buffer.copy_(p0)
        psgd._powersgd._qs_buffer.copy_(q0)
        psgd.step_counter = psgd._powersgd.step_counter = 0
        gd = [g.to(DEV) for g in grads]
        od = psgd.aggregate(gd)
        torch.cuda.synchronize()
        runs.append([o.clone() for o in od] + [g.clone() for g in gd] +
                    [psgd._powersgd._ps_buffer.clone(), psgd._powersgd._qs_buffer.clone()])
    for x, y in zip(runs[0], runs[1]):
        assert torch.equal(x, y)


def test_is_wide_query():
    for rank, wide in ((32, False), (33, True), (64, True), (128, True)):
        plan = PowerSGD([torch.zeros(s, device=DEV) for s in SHAPES_A], Config(rank, 0.1, 2, 0))._powersgd._plan
        assert plan.is_wide() == wide
        if wide:
            assert all(plan.fused_final(step, agg) == 0 for step in range(4) for agg in (False, True))


def test_refusals_leave_everything_untouched():
    shapes = [s for s in SHAPES_A if len(s) > 1]
    plan = _lib.Plan(shapes, 64, 2, _lib.PSGD_F32)
    pn, qn = plan.factor_numel()
    gen = torch.Generator().manual_seed(3)
    P = torch.randn(pn, generator=gen).to(DEV)
    Q = torch.randn(qn, generator=gen).to(DEV)
    ws = torch.empty(plan.workspace_bytes(), dtype=torch.uint8, device=DEV)
    plan.bind(0, P.data_ptr(), Q.data_ptr(), ws.data_ptr())
    grads = [torch.from_numpy(f).to(DEV) for f in hash_tensors(shapes, seed=9)]
    outs = [torch.zeros_like(g) for g in grads]
    flat_out = torch.zeros(sum(g.numel() for g in grads), device=DEV)
    keep = [g.clone() for g in grads] + [P.clone(), Q.clone()]
    ptrs = _lib.ptr_array([g.data_ptr() for g in grads])
    optrs = _lib.ptr_array([o.data_ptr() for o in outs])
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(max(pn, qn), device=DEV)
    y = torch.zeros(max(pn, qn), device=DEV)
    msg = "ranks above 32 are not supported there"
    with pytest.raises(ValueError, match=msg):
        plan.product(ptrs, False, x.data_ptr(), y.data_ptr(), (), stream)
    with pytest.raises(ValueError, match=msg):
        plan.orthogonalize(True, P.data_ptr(), 0, stream)
    with pytest.raises(ValueError, match=msg):
        plan.reconstruct(ptrs, None, optrs, [(P.data_ptr(), Q.data_ptr())], [(P.data_ptr(), Q.data_ptr())], 1.0, stream)
    with pytest.raises(ValueError, match="ranks above 32"):
        plan.set_buckets([2, len(plan.groups())])
    with pytest.raises(ValueError, match=msg):
        plan.compress_bucket(ptrs, 0, 0, 0, stream)
    with pytest.raises(ValueError, match=msg):
        plan.decompress_bucket(ptrs, flat_out.data_ptr(), 0, 1, 0, stream)
    with pytest.raises(ValueError, match=msg):
        plan.ipc_create(0)
    red = RankKReducer(random_seed=1, device=DEV, rank=64)
    mem = [torch.zeros_like(g) for g in grads]
    with pytest.raises(ValueError, match=msg):
        red.reduce([g for g in grads], outs, mem)
    torch.cuda.synchronize()
    for a, b in zip(keep, grads + [P, Q]):
        assert torch.equal(a, b)
    assert not bool(y.any()) and not any(bool(o.any()) for o in outs) and not bool(flat_out.any())
