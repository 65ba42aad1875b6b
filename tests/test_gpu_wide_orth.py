"""The wide-rank orthonormalisation (k_wide_gram -> k_wide_chol -> k_wide_orth_apply,
psgd_wide.hip; effective ranks 33-128) pinned one launch at a time: ONE psgd_compress call on a
plan whose in-factor buffer holds crafted panels, then the in-factor buffer (now X_hat) and the
out-factor buffer (G^T X_hat or G X_hat) are read back. step = 0 orthonormalises the P panels,
step = 1 the Q panels (parity (step * iters + it) % 2 with iters = 1).

References, per fp32 panel X: Q64 = torch.linalg.qr(X.double()).Q (LAPACK's column signs, high
precision) and Q32 = the oracle's orthonormalise_ of the fp32 panel (the reference's own result).
With e_ref[j] = ||Q32[:, j] - Q64[:, j]||_2 a kernel column must satisfy

    ||X_hat[:, j] - Q64[:, j]||_2 <= max(1e-5, 8 * e_ref[j]):

the floor is the project's tolerance for orthonormal columns (test_gpu_orth.py), the factor 8 is
headroom for a different summation order of the same algorithm in the same precision; a wrong
reflector, sign or Gram slot is an O(1) error. Every panel is also checked for finite entries,
max |X_hat^T X_hat - I| <= 1e-5 in fp64, and the product left in the out-factor buffer against the
fp64 product with the GPU's own X_hat within 1e-6 of ||G||_F ||X_hat||_F, which proves that the
history copy the product reads equals the state. Every comparison goes through parity_log.check;
DESIGN.md section 5 quotes the observed values."""
import pytest
import torch

from oracle import powersgd_oracle as O
from parity_log import check
from powersgd_amd import Config, PowerSGD, _lib
from powersgd_amd.workloads import hash_tensors
from test_gpu_orth import _structure_
from test_gpu_wide_rank import _panels

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

TOL_COL = 1e-5    # floor of the per-column bound
REF_FACTOR = 8.0  # headroom over the reference's own fp32 error
TOL_ORTH = 1e-5   # max |X^T X - I|
TOL_PROD = 1e-6   # product against ||G||_F ||X_hat||_F
TOL_RANGE = 1e-5  # range containment of a rank-deficient panel
PIVOT_RULE = 1e-8  # k_wide_chol rejects a pivot at or below this fraction of the squared norm


# ----------------------------------------------------------------------- driver --
class _Panel:
    """One in-factor panel of a launch: x the crafted input [k, r], xh the GPU's result, g the
    matrix [n, m], y the out-factor panel the same launch left."""

    def __init__(self, x, xh, g, y, even):
        self.x, self.xh, self.g, self.y, self.even = x, xh, g, y, even
        self.k, self.r = x.shape


def _launch(shapes, rank, step, craft, seed):
    """One compress call. ``craft(i, panel, gen)`` rewrites in-side panel i in place (plan order:
    shape groups in first-appearance order, the matrices of a group in tensor order)."""
    plan = _lib.Plan(shapes, rank, 1, _lib.PSGD_F32)
    assert plan.is_wide()
    groups = plan.groups()
    pn, qn = plan.factor_numel()
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(pn, generator=gen)
    q0 = torch.randn(qn, generator=gen)
    grads = [torch.randn(s, generator=gen) for s in shapes]
    even = step % 2 == 0
    side = 0 if even else 1
    xin = _panels(p0 if even else q0, groups, side)
    for i, v in enumerate(xin):
        craft(i, v, gen)
    x0 = [v.clone() for v in xin]
    P, Q = p0.to(DEV), q0.to(DEV)
    ws = torch.empty(plan.workspace_bytes(), dtype=torch.uint8, device=DEV)
    plan.bind(0, P.data_ptr(), Q.data_ptr(), ws.data_ptr())
    gd = [g.to(DEV) for g in grads]
    plan.compress(_lib.ptr_array([g.data_ptr() for g in gd]), step, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ph, qh = P.cpu(), Q.cpu()
    xh = _panels(ph if even else qh, groups, side)
    yh = _panels(qh if even else ph, groups, 1 - side)
    order = [t for n, m, _, _ in groups for t, s in enumerate(shapes) if tuple(s) == (n, m)]
    assert len(order) == len(shapes) == len(xh)
    return [_Panel(x0[i], xh[i], grads[t], yh[i], even) for i, t in enumerate(order)]


# ------------------------------------------------------------------- assertions --
def _assert_product(tag, p):
    """Finite, and the out-factor panel is the product with the GPU's own X_hat."""
    assert bool(torch.isfinite(p.xh).all()) and bool(torch.isfinite(p.y).all()), tag
    g, xh = p.g.double(), p.xh.double()
    want = g.t() @ xh if p.even else g @ xh
    err = float((p.y.double() - want).norm()) / (float(g.norm() * xh.norm()) + 1e-30)
    check(err, TOL_PROD, *tag, "product")


def _assert_orthonormal(tag, p):
    xh = p.xh.double()
    dev = float((xh.t() @ xh - torch.eye(p.r, dtype=torch.float64)).abs().max())
    check(dev, TOL_ORTH, *tag, "orthonormal")


def _references(x):
    q64 = torch.linalg.qr(x.double()).Q
    q32 = x.clone().unsqueeze(0)
    O.orthonormalise_(q32)
    return q64, q32[0]


def _assert_columns(tag, p, ncols=None):
    """The per-column bound over the leading ``ncols`` columns (default all). Logs the column
    closest to its bound, with e_ref of that column and the largest error / e_ref of the panel, and
    the column with the largest error."""
    q64, q32 = _references(p.x)
    n = p.r if ncols is None else ncols
    e_ref = (q32.double() - q64).norm(dim=0)[:n]
    err = (p.xh.double() - q64).norm(dim=0)[:n]
    bound = torch.clamp(REF_FACTOR * e_ref, min=TOL_COL)
    j = int((err / bound).argmax())
    ratio = float((err / e_ref.clamp(min=1e-30)).max())
    print(f"{tag}: worst column {j} err {float(err[j]):.3e} bound {float(bound[j]):.3e} "
          f"e_ref {float(e_ref[j]):.3e} max err/e_ref {ratio:.2f}")
    check(float(err[j]), float(bound[j]), *tag, "column", j, f"e_ref={float(e_ref[j]):.3e}", f"ratio={ratio:.3f}")
    j = int(err.argmax())  # and the largest error, which is another column where e_ref varies
    check(float(err[j]), float(bound[j]), *tag, "column-max", j, f"e_ref={float(e_ref[j]):.3e}")
    assert bool((err <= bound).all()), (tag, err, bound)


def _assert_full_rank(tag, p):
    _assert_product(tag, p)
    _assert_orthonormal(tag, p)
    _assert_columns(tag, p)


def _assert_trapezoid(tag, p):
    """LAPACK leaves every column of an upper-trapezoidal panel unreflected: exactly I[:, :r]."""
    _assert_product(tag, p)
    _assert_orthonormal(tag, p)
    eye = torch.eye(p.k, p.r, dtype=torch.float64)
    assert float((torch.linalg.qr(p.x.double()).Q - eye).abs().max()) <= 1e-14, tag  # the input is what it claims
    check(float((p.xh.double() - eye).norm(dim=0).max()), 1e-6, *tag, "identity")


def _assert_deficient(tag, p):
    """Duplicated columns: the trailing half is decided by rounding in LAPACK itself."""
    _assert_product(tag, p)
    _assert_orthonormal(tag, p)
    _assert_columns(tag, p, ncols=p.r // 2)
    x, xh = p.x.double(), p.xh.double()
    check(float((x - xh @ (xh.t() @ x)).norm()) / float(x.norm()), TOL_RANGE, *tag, "range")


def _assert_rank1(tag, panels):
    """A rank-1 shape group is divided by its joint norm (the oracle's orthonormalise_ of the
    [B, k, 1] batch)."""
    want = torch.stack([p.x for p in panels])
    O.orthonormalise_(want)
    got = torch.stack([p.xh for p in panels])
    for p in panels:
        _assert_product(tag, p)
    check(float((got.double() - want.double()).norm()) / float(want.double().norm()), 1e-6, *tag, "joint-norm")


# -------------------------------------------------------------------- crafting --
def _deficient_(v, gen):
    rho = v.shape[1] // 2
    v[:, rho:2 * rho] = v[:, :rho]
    v[:, 2 * rho:] = 0.0


def _near_dependent_(v, gen, delta):
    """Last column = c + delta ||c|| u: c a random combination of the others, u the direction of
    the original last column (fp64, rounded to fp32 once)."""
    x = v.double()
    w = torch.randn(v.shape[1] - 1, generator=gen, dtype=torch.float64)
    c = x[:, :-1] @ w
    u = x[:, -1] / x[:, -1].norm()
    v[:, -1] = (c + delta * c.norm() * u).float()


def _last_pivot_ratio(x):
    """Last Cholesky pivot of X^T X over the column's squared norm, in fp64."""
    gram = x.double().t() @ x.double()
    return float(torch.linalg.cholesky(gram, upper=True)[-1, -1]) ** 2 / float(gram[-1, -1])


def _single(kind, k, r, side, check_fn, craft=None):
    """A single-matrix plan: side P = shape (k, r), step 0; side Q = shape (r, k), step 1: the
    crafted [k, r] panel is the in-factor either way."""
    shape, step = ((k, r), 0) if side == "P" else ((r, k), 1)
    seed = 7919 * k + 101 * r + step + 17 * sum(map(ord, kind))
    (p,) = _launch([shape], r, step, (lambda i, v, gen: craft(v, gen)) if craft else (lambda i, v, gen: None), seed)
    assert (p.k, p.r) == (k, r)
    check_fn((kind, k, r, side), p)
    return p


def _ids(cases):
    return ["-".join(str(c) for c in case) for case in cases]


SIDES = ("P", "Q")
RAGGED_R = (33, 47, 50, 64, 65, 97, 127, 128)

# --------------------------------------------------- 1. full-rank random panels --
RANDOM_CASES = ([("gram-edge", k, r, s) for k in (511, 512, 513, 1024, 1025) for r in (33, 64, 65, 128) for s in SIDES] +
                [("ragged", 200, r, s) for r in RAGGED_R for s in SIDES] +
                [("square", r, r, s) for r in RAGGED_R for s in SIDES])


@pytest.mark.parametrize("kind,k,r,side", RANDOM_CASES, ids=_ids(RANDOM_CASES))
def test_random_panel_columns_match_lapack(kind, k, r, side):
    """Cholesky-QR with LAPACK's signs: panels at each side of the 512-row Gram blocks, r off the
    multiples of 4 and 16 inside the 64 / 128 column instances, and square panels (the j == k - 1
    sign rule), on both the P and the Q side."""
    _single(kind, k, r, side, _assert_full_rank)


# -------------------------------- 2. structured panels: the Householder fallback --
STRUCT_CASES = [(kind, k, r, s) for kind in ("trapezoid", "col0") for r in (33, 64, 100, 128)
                for k in (r, 200, 513) for s in SIDES]


@pytest.mark.parametrize("kind,k,r,side", STRUCT_CASES, ids=_ids(STRUCT_CASES))
def test_unreflected_columns_take_the_fallback(kind, k, r, side):
    """Sign pivots within kSignTol of 1 divert the panel to wide_householder. trapezoid: every
    column unreflected, exactly I[:, :r]; col0: column 0 = -2 e_0 is kept as +e_0 and every other
    column goes through a real reflection (wide_reflect in geqr2 and org2r)."""
    _single(kind, k, r, side, _assert_trapezoid if kind == "trapezoid" else _assert_full_rank,
            craft=lambda v, gen: _structure_(v.unsqueeze(0), kind, r))


# ----------------------------------------- 3. rank-deficient, non-zero panels --
DEFICIENT_CASES = [("deficient", k, r, s) for r in (34, 64, 128) for k in (200, 513) for s in SIDES]


@pytest.mark.parametrize("kind,k,r,side", DEFICIENT_CASES, ids=_ids(DEFICIENT_CASES))
def test_duplicated_columns(kind, k, r, side):
    """Columns rho .. 2 rho - 1 are bit-for-bit copies of columns 0 .. rho - 1 (rho = r // 2): a
    zero Cholesky pivot, the fallback, and reflections on rounding noise. The leading rho columns
    depend only on the first reflectors; the rest must still complete an orthonormal basis whose
    range holds the panel."""
    _single(kind, k, r, side, _assert_deficient, craft=_deficient_)


# ------------------------------------- 4. both sides of the rejection threshold --
ACCEPTED = (1e-1, 1e-2, 1e-3)
REJECTED = (3e-5, 1e-6)
THRESHOLD_CASES = [(f"delta{d:g}", k, r, s) for d in ACCEPTED + REJECTED for k in (200, 513) for r in (33, 64, 128)
                   for s in SIDES]


@pytest.mark.parametrize("kind,k,r,side", THRESHOLD_CASES, ids=_ids(THRESHOLD_CASES))
def test_rejection_threshold(kind, k, r, side):
    """The last column within delta of the span of the others. delta >= 1e-3 stays above the
    1e-8 pivot rule (Cholesky-QR at its worst conditioning), delta <= 3e-5 falls below it (the
    fallback); which side a panel is on is asserted on the input, in fp64, with a factor 10 to
    spare. e_ref of the last column grows as the panel degenerates and the bound follows it."""
    delta = float(kind[len("delta"):])

    def verify(tag, p):
        ratio = _last_pivot_ratio(p.x)
        print(f"{tag}: last pivot / squared norm {ratio:.3e}")
        if delta in ACCEPTED:
            assert ratio >= 10 * PIVOT_RULE, (tag, ratio)
        else:
            assert ratio <= PIVOT_RULE / 10, (tag, ratio)
        _assert_full_rank(tag, p)

    _single(kind, k, r, side, verify, craft=lambda v, gen: _near_dependent_(v, gen, delta))


# ------------------------------------------------------------ 5. mixed launch --
MIXED = {
    64: [(200, 64), (200, 64), (64, 1100), (300, 16), (200, 1), (130, 70), (130, 70)],
    128: [(300, 128), (300, 128), (128, 1100), (300, 16), (200, 1), (260, 140), (260, 140)],
}
MIXED_KINDS = ["col0", "random", "random", "narrow", "rank1", "deficient", "random"]


@pytest.mark.parametrize("rank", [64, 128])
@pytest.mark.parametrize("step", [0, 1], ids=["P", "Q"])
def test_mixed_launch(rank, step):
    """The per-unit ok gate of k_wide_orth_apply and the per-side Gram slots: one launch with a
    rejected col0 panel beside an accepted one, a 3-block panel on the Q side only (slot counts
    differ per side), an r = 16 unit, a rank-1 unit (joint norm) and a duplicate-deficient panel
    beside an accepted one. Every panel meets its own kind's assertions."""
    shapes = MIXED[rank]

    def craft(i, v, gen):
        if MIXED_KINDS[i] == "col0":
            _structure_(v.unsqueeze(0), "col0", v.shape[1])
        elif MIXED_KINDS[i] == "deficient":
            _deficient_(v, gen)

    panels = _launch(shapes, rank, step, craft, 4242 + 2 * rank + step)
    assert [p.r for p in panels] == [rank, rank, rank, 16, 1, rank, rank]
    for i, (kind, p) in enumerate(zip(MIXED_KINDS, panels)):
        tag = ("mixed", rank, "PQ"[step], i, kind, p.k, p.r)
        if kind == "rank1":
            _assert_rank1(tag, [p])
        elif kind == "deficient":
            _assert_deficient(tag, p)
        else:
            _assert_full_rank(tag, p)


# ----------------------------- 6. rank-deficient factors through the real step --
@pytest.mark.parametrize("rank", [64, 128])
def test_zero_and_rank_deficient_panels(rank):
    """test_gpu_orth.py's case at ranks 64 / 128, through the Python front end: zero gradients
    make the next factor zero (fallback: identity columns), a rank-1 gradient u v^T makes it rank
    deficient; the completion columns are orthogonal to u, so outputs and residuals are well posed."""
    shapes = [(160, 136), (160, 136), (300, 200)]
    psgd = PowerSGD([torch.zeros(s, device=DEV) for s in shapes], Config(rank, 0.1, 2, 0))
    assert psgd._powersgd._plan.is_wide()
    ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 0.1, 2, 0)
    ora.codec.p_flat.copy_(psgd._powersgd._ps_buffer.cpu())
    ora.codec.q_flat.copy_(psgd._powersgd._qs_buffer.cpu())
    u = torch.from_numpy(hash_tensors([(300, 1)], seed=3)[0])
    v = torch.from_numpy(hash_tensors([(1, 200)], seed=4)[0])
    g = [torch.zeros(160, 136), torch.zeros(160, 136), u @ v]
    for t in range(2):
        gd = [x.to(DEV) for x in g]
        gc = [x.clone() for x in g]
        outs = psgd.aggregate(gd)
        oc = O.policy_step(ora, gc)
        torch.cuda.synchronize()
        for i, x in enumerate(g):
            scale = max(float(x.norm()), 1.0)
            assert bool(torch.isfinite(outs[i]).all()) and bool(torch.isfinite(gd[i]).all())
            check(float((outs[i].cpu() - oc[i]).norm()) / scale, 1e-5, "deficient-step", rank, t, i, "out")
            check(float((gd[i].cpu() - gc[i]).norm()) / scale, 1e-5, "deficient-step", rank, t, i, "res")
        g = [r.cpu() + x for r, x in zip(gd, g)]
