"""The mixed-dtype run-table kernels (psgd_runs_create_mixed: bf16 bucket side, fp32 tensors)
through ``_lib.Runs``, in the single-bucket form (a DDP bucket) and the source-table form (the
``optimizer_step`` flow's separate gradient tensors).

Both passes are exact by construction, so every check is bitwise: ADD is one fp32 add of an
exactly upcast bf16 value (``before + bucket.float()``), GATHER one round-to-nearest-even
conversion (``tensor.bfloat16()``). Run lengths straddle the work-item size (kRunItem = 4096);
both sides use odd element offsets (2-byte / 4-byte alignment only), two runs share a tensor,
one tensor is touched by no run, and canary-filled gaps separate the runs on both sides."""
import ctypes

import pytest
import torch

from powersgd_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16 = _lib.PSGD_F32, _lib.PSGD_BF16
K = 4096  # kRunItem (csrc/psgd_internal.h)
LENS = [1, 7, K - 1, K, K + 1, 3 * K + 5]
# run k: (tensor, tensor offset); tensor 0 takes two runs, tensor 2 none
TENSOR = [0, 0, 1, 3, 4, 5]
TOFF = [3, 9, 1, 5, 0, 7]
TSIZE = [20, K + 3, 64, K + 9, K + 4, 3 * K + 15]
# single-bucket form: bucket offsets with gaps (odd and even starts)
BOFF, _o = [], 1
for _n in LENS:
    BOFF.append(_o)
    _o += _n + 3
BSIZE = _o + 2
# source-table form: run k lives in source SRC[k] at offset SOFF[k]; source 0 takes two runs, 2 none
SRC = [0, 0, 1, 3, 4, 5]
SOFF = [1, 11, 3, 0, 5, 1]
SSIZE = [24, K + 5, 16, K + 2, K + 9, 3 * K + 9]
T_CANARY, B_CANARY = 555.0, 777.0
assert any(o % 2 for o in BOFF) and any(o % 2 for o in TOFF) and any(o % 2 for o in SOFF)


class _Table:
    def __init__(self, tcode, bcode=None, listed=False, boff=None):
        n = len(LENS)
        kw = dict(source=SRC, nsources=len(SSIZE)) if listed else {}
        self.runs = _lib.Runs(boff or (SOFF if listed else BOFF), TENSOR, TOFF, LENS, len(TSIZE), tcode, bcode, **kw)
        self.ws = torch.empty(self.runs.workspace_bytes(), dtype=torch.uint8, device=DEV)
        self.runs.bind(0, self.ws.data_ptr())
        assert n == len(TENSOR) == len(TOFF)


def _ptrs(ts):
    return _lib.ptr_array([t.data_ptr() for t in ts])


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tensors(seed, special=False):
    """fp32 tensors (CPU): canary everywhere, seeded normals under the runs."""
    g = _gen(seed)
    ts = [torch.full((n,), T_CANARY) for n in TSIZE]
    for k, n in enumerate(LENS):
        ts[TENSOR[k]][TOFF[k]:TOFF[k] + n] = torch.randn(n, generator=g)
    if special:
        sp = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38, -3.4e38,
                           3.3895313892515355e38, -3.3895313892515355e38, float("nan")])
        k = len(LENS) - 1  # the longest run: specials at its start and across its second work item
        ts[TENSOR[k]][TOFF[k]:TOFF[k] + len(sp)] = sp
        ts[TENSOR[k]][TOFF[k] + K - 3:TOFF[k] + K - 3 + len(sp)] = sp
    return ts


def _bucket_sides(seed, listed):
    """bf16 bucket side (CPU): one buffer, or the list of sources; canary in the gaps."""
    g = _gen(seed)
    if not listed:
        b = torch.full((BSIZE,), B_CANARY).bfloat16()
        for k, n in enumerate(LENS):
            b[BOFF[k]:BOFF[k] + n] = torch.randn(n, generator=g).bfloat16()
        return [b]
    ss = [torch.full((n,), B_CANARY).bfloat16() for n in SSIZE]
    for k, n in enumerate(LENS):
        ss[SRC[k]][SOFF[k]:SOFF[k] + n] = torch.randn(n, generator=g).bfloat16()
    return ss


def _slices(listed):
    """Per run: (bucket-side tensor index, bucket-side offset)."""
    return list(zip(SRC, SOFF)) if listed else [(0, o) for o in BOFF]


def _bits(x):
    return x.view(torch.int16)


@pytest.mark.parametrize("listed,zero", [(False, False), (True, False), (True, True)])
def test_add_is_one_fp32_add(listed, zero):
    before = _tensors(1)
    side = _bucket_sides(2, listed)
    want = [t.clone() for t in before]
    want_side = [s.clone() for s in side]
    for k, (n, (si, so)) in enumerate(zip(LENS, _slices(listed))):
        want[TENSOR[k]][TOFF[k]:TOFF[k] + n] += side[si][so:so + n].float()
        if zero:
            want_side[si][so:so + n] = 0
    ts = [t.to(DEV) for t in before]
    bs = [s.to(DEV) for s in side]
    tab = _Table(F32, BF16, listed)
    tp = _ptrs(ts)
    if listed:
        tab.runs.add_list(_ptrs(bs), tp, zero, _stream())
    else:
        tab.runs.add(bs[0].data_ptr(), tp, _stream())
    torch.cuda.synchronize()
    for i, (a, w) in enumerate(zip(ts, want)):
        assert torch.equal(a.cpu(), w), i  # the sums, the gaps' canaries, the untouched tensor
    assert torch.equal(ts[2].cpu(), torch.full((TSIZE[2],), T_CANARY))
    for i, (a, w) in enumerate(zip(bs, want_side)):
        assert torch.equal(_bits(a.cpu()), _bits(w)), i  # sources: +0.0 under the runs, gaps unchanged


@pytest.mark.parametrize("listed", [False, True])
def test_gather_rounds_to_nearest_even(listed):
    src = _tensors(3, special=True)
    side = _bucket_sides(4, listed)
    want = [s.clone() for s in side]
    nan = [torch.zeros(s.shape, dtype=torch.bool) for s in side]
    for k, (n, (si, so)) in enumerate(zip(LENS, _slices(listed))):
        x = src[TENSOR[k]][TOFF[k]:TOFF[k] + n]
        want[si][so:so + n] = x.bfloat16()
        nan[si][so:so + n] = x.isnan()
    # the conversion's fixed points (ties to even, overflow to inf, the largest finite bf16)
    probe = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38, 3.3895313892515355e38]).bfloat16().float()
    assert probe.tolist() == [1.0, 1.015625, float("inf"), 3.3895313892515355e38]
    ts = [t.to(DEV) for t in src]
    bs = [s.to(DEV) for s in side]
    tab = _Table(F32, BF16, listed)
    if listed:
        tab.runs.gather_list(_ptrs(bs), _ptrs(ts), _stream())
    else:
        tab.runs.gather(bs[0].data_ptr(), _ptrs(ts), _stream())
    torch.cuda.synchronize()
    assert sum(int(m.sum()) for m in nan) == 2
    for i, (a, w, m) in enumerate(zip(bs, want, nan)):
        a = a.cpu()
        assert bool(a[m].isnan().all()), i
        assert torch.equal(_bits(a)[~m], _bits(w)[~m]), i  # bit for bit, canary gaps included
    for a, b in zip(ts, src):  # the tensors are read only
        a = a.cpu()
        assert torch.equal(a[~a.isnan()], b[~b.isnan()])


def test_equal_pairs_in_the_source_table_form():
    """The source-table form with one dtype on both sides keeps k_runs' arithmetic (bf16: an fp32
    add rounded to nearest even)."""
    for code, dt in ((F32, torch.float32), (BF16, torch.bfloat16)):
        before = [t.to(dt) for t in _tensors(5)]
        side = [s.to(dt) for s in _bucket_sides(6, True)]
        want = [t.clone() for t in before]
        for k, (n, (si, so)) in enumerate(zip(LENS, _slices(True))):
            sl = slice(TOFF[k], TOFF[k] + n)
            want[TENSOR[k]][sl] = (want[TENSOR[k]][sl].float() + side[si][so:so + n].float()).to(dt)
        ts = [t.to(DEV) for t in before]
        bs = [s.to(DEV) for s in side]
        tab = _Table(code, code, True)
        tab.runs.add_list(_ptrs(bs), _ptrs(ts), False, _stream())
        torch.cuda.synchronize()
        for i, (a, w) in enumerate(zip(ts, want)):
            assert torch.equal(a.cpu(), w), (dt, i)
        for a, w in zip(bs, side):
            assert torch.equal(a.cpu(), w)


def test_fp32_residual_does_not_stagnate():
    """tensor = 1.0, bucket = 2^-10, eight ADDs: the fp32 tensors reach 1 + 8 * 2^-10 exactly; a
    bf16 table on the same data stays at 1.0 (each sum rounds back to 1.0, nearest even)."""
    bucket = torch.full((BSIZE,), 2.0 ** -10, dtype=torch.bfloat16, device=DEV)
    for code, dt, want in ((F32, torch.float32, 1.0078125), (BF16, torch.bfloat16, 1.0)):
        ts = [torch.ones(n, dtype=dt, device=DEV) for n in TSIZE]
        tab = _Table(code, BF16)
        tp = _ptrs(ts)
        for _ in range(8):
            tab.runs.add(bucket.data_ptr(), tp, _stream())
        torch.cuda.synchronize()
        for k, n in enumerate(LENS):
            got = ts[TENSOR[k]][TOFF[k]:TOFF[k] + n].float().cpu()
            assert torch.equal(got, torch.full((n,), want)), (dt, k)
        assert torch.equal(ts[2].float().cpu(), torch.ones(TSIZE[2]))


def test_wrong_form_is_refused_without_a_launch():
    ts = [torch.zeros(n, device=DEV) for n in TSIZE]
    b = torch.zeros(BSIZE, dtype=torch.bfloat16, device=DEV)
    one, lst = _Table(F32, BF16, False), _Table(F32, BF16, True)
    with pytest.raises(RuntimeError, match="STATE"):
        one.runs.add_list(_ptrs([b] * len(SSIZE)), _ptrs(ts), False, _stream())
    with pytest.raises(RuntimeError, match="STATE"):
        lst.runs.gather(b.data_ptr(), _ptrs(ts), _stream())
    torch.cuda.synchronize()
    assert not bool(b.any()) and not any(bool(t.any()) for t in ts)
