"""Host side of the wide-rank path (effective ranks 33-128, fp32 / bf16): plan creation, layout
queries against the oracle, the rank limits, and the unchanged rank-32 plan. No GPU compute."""
import pytest
import torch

from oracle import powersgd_oracle as O
from powersgd_amd import _lib

# narrow, masked and rank-1 matrices inside a wide plan
SHAPES_N = [(300, 200), (64, 1000), (1000, 48), (129, 67), (77, 130), (1000, 16), (200, 1), (128, 8, 3, 3)]


def _matrix(shape):
    n = shape[0]
    numel = 1
    for d in shape:
        numel *= d
    return n, numel // n


@pytest.mark.parametrize("dtype", [_lib.PSGD_F32, _lib.PSGD_BF16])
@pytest.mark.parametrize("rank", [33, 64, 128])
def test_wide_plan_layout_matches_reference(rank, dtype):
    iters = 2
    plan = _lib.Plan(SHAPES_N, rank, iters, dtype)
    assert plan.is_wide()
    groups = plan.groups()
    mats = [_matrix(s) for s in SHAPES_N]
    assert [(n, m) for n, m, _, _ in groups] == mats  # every shape of set N is its own group
    assert [r for _, _, r, _ in groups] == [min(rank, n, m) for n, m in mats]
    assert plan.factor_numel() == (sum(c * n * r for n, _, r, c in groups), sum(c * m * r for _, m, r, c in groups))
    assert plan.workspace_bytes() > 0
    st = O.codec_init([torch.zeros(s) for s in SHAPES_N], rank, iters)
    assert plan.factor_numel() == (st.p_flat.numel(), st.q_flat.numel())
    rate, _unc, _comp = plan.compression_rate()
    assert rate == pytest.approx(O.codec_compression_rate(st), rel=1e-12)
    for step in range(3):
        assert plan.fused_final(step, True) == 0 and plan.fused_final(step, False) == 0
        assert not any(plan.odd_even(step, it) for it in range(iters))


def test_rank_limits():
    with pytest.raises(ValueError, match="128"):
        _lib.Plan(SHAPES_N, 129, 2, _lib.PSGD_F32)
    with pytest.raises(ValueError, match="128"):
        _lib.Plan([(300, 200)], 200, 1, _lib.PSGD_BF16)
    with pytest.raises(ValueError, match="32"):
        _lib.Plan(SHAPES_N, 64, 2, _lib.PSGD_F64)
    # the limit is on the EFFECTIVE rank: a large rank on small matrices is a narrow plan
    assert not _lib.Plan([(20, 30), (8, 100)], 500, 2, _lib.PSGD_F32).is_wide()
    assert _lib.Plan([(20, 30), (8, 100)], 500, 2, _lib.PSGD_F64).groups()[0][2] == 20


def test_one_bucket_only():
    plan = _lib.Plan(SHAPES_N, 64, 2, _lib.PSGD_F32)
    plan.set_buckets([len(SHAPES_N)])
    with pytest.raises(ValueError, match="ranks above 32"):
        plan.set_buckets([3, len(SHAPES_N)])


# workspace of the rank-32 plan over set N as the library laid it out before the wide path
# existed: the wide path must not move anything in a plan it does not serve
RANK32_WORKSPACE = {_lib.PSGD_F32: 4852480, _lib.PSGD_BF16: 4852480}


@pytest.mark.parametrize("dtype", [_lib.PSGD_F32, _lib.PSGD_BF16])
def test_rank32_plan_unchanged(dtype, monkeypatch):
    # (the default of this knob is an occupancy query, which needs a device: pin it)
    monkeypatch.setenv("PSGD_EVEN_WPC", "2")
    plan = _lib.Plan(SHAPES_N, 32, 2, dtype)
    assert not plan.is_wide()
    assert plan.workspace_bytes() == RANK32_WORKSPACE[dtype]
    assert [r for _, _, r, _ in plan.groups()] == [min(32, *_matrix(s)) for s in SHAPES_N]
