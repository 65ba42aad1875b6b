"""Host-side contract of the mixed-dtype / source-table run tables (include/psgd.h
``psgd_runs_create_mixed``, ``psgd_runs_add_list``, ``psgd_runs_gather_list``) and of
``PowerSGDState(residual_dtype=...)``'s argument check. No GPU: nothing here binds or launches."""
import ctypes
import itertools

import pytest
import torch

from powersgd_amd import _lib

F32, BF16, F64 = _lib.PSGD_F32, _lib.PSGD_BF16, _lib.PSGD_F64
OK, VALUE, DTYPE, STATE = 0, 2, 3, 6
_i32, _i64 = ctypes.c_int32, ctypes.c_int64


def _create(bdt, tdt, source=None, nsources=0, boff=(0,), tensor=(0,), toff=(0,), length=(5,), nruns=None,
            ntensors=1, out=True):
    n = len(length) if nruns is None else nruns
    arr = lambda ty, xs: None if xs is None else (ty * max(1, len(xs)))(*xs)
    h = ctypes.c_void_p()
    st = _lib.lib().psgd_runs_create_mixed(arr(_i64, boff), arr(_i32, tensor), arr(_i64, toff), arr(_i64, length),
                                           arr(_i32, source), n, ntensors, nsources, bdt, tdt,
                                           ctypes.byref(h) if out else None)
    return st, h


def _destroy(h):
    if h.value:
        _lib.lib().psgd_runs_destroy(h)


ACCEPTED = {(F32, F32), (BF16, BF16), (F64, F64), (BF16, F32)}


@pytest.mark.parametrize("source", [None, (0,)])
@pytest.mark.parametrize("bdt,tdt", list(itertools.product((F32, BF16, F64, 3, -1), repeat=2)))
def test_dtype_pairs(bdt, tdt, source):
    st, h = _create(bdt, tdt, source=source, nsources=1)
    try:
        if (bdt, tdt) in ACCEPTED:
            assert st == OK and h.value
        else:
            assert st == DTYPE and not h.value
            assert b"dtype" in _lib.lib().psgd_last_error()
    finally:
        _destroy(h)


def test_null_and_negative_arguments_are_refused_like_psgd_runs_create():
    assert _create(BF16, F32, out=False)[0] == VALUE
    for kw in (dict(boff=None), dict(tensor=None), dict(toff=None), dict(length=None, nruns=1)):
        st, h = _create(BF16, F32, **kw)
        assert st == VALUE and not h.value, kw
    for kw in (dict(nruns=-1), dict(ntensors=-1), dict(nsources=-1), dict(length=(-1,)), dict(boff=(-1,)),
               dict(toff=(-2,)), dict(tensor=(-1,)), dict(tensor=(1,)),
               dict(source=(-1,), nsources=1), dict(source=(1,), nsources=1), dict(source=(0,), nsources=0)):
        st, h = _create(BF16, F32, **kw)
        assert st == VALUE and not h.value, kw
    # a bad table is reported before a bad dtype, as psgd_runs_create orders its checks
    assert _create(F32, BF16, nruns=-1)[0] == VALUE
    # empty tables are fine (no runs: the arrays may be null)
    st, h = _create(BF16, F32, boff=None, tensor=None, toff=None, length=None, nruns=0, ntensors=0)
    assert st == OK
    _destroy(h)


def test_compute_before_bind_is_a_state_error():
    L = lib = _lib.lib()
    dummy = (ctypes.c_void_p * 1)(0x1000)  # never dereferenced: the table is not bound
    st, h = _create(BF16, F32)
    try:
        assert L.psgd_runs_add(h, 0x1000, dummy, None) == STATE
        assert L.psgd_runs_gather(h, 0x1000, dummy, None) == STATE
    finally:
        _destroy(h)
    st, h = _create(BF16, F32, source=(0,), nsources=1)
    try:
        assert lib.psgd_runs_add_list(h, dummy, dummy, 1, None) == STATE
        assert lib.psgd_runs_gather_list(h, dummy, dummy, None) == STATE
        assert b"not bound" in lib.psgd_last_error()
        # the other form's entry points refuse the table whatever its state
        assert lib.psgd_runs_add(h, 0x1000, dummy, None) == STATE
        assert lib.psgd_runs_gather_list(None, dummy, dummy, None) == VALUE
    finally:
        _destroy(h)


def test_workspace_holds_both_pointer_tables():
    def ws(**kw):
        st, h = _create(BF16, F32, **kw)
        assert st == OK
        b = _i64()
        assert _lib.lib().psgd_runs_workspace_bytes(h, ctypes.byref(b)) == OK
        _destroy(h)
        return b.value

    assert ws(source=(0,), nsources=1) > ws()


def test_runs_binding_routes_optional_arguments():
    _lib.Runs([0], [0], [0], [4], 1, F32)  # existing callers: psgd_runs_create
    _lib.Runs([0], [0], [0], [4], 1, F32, BF16)
    _lib.Runs([0], [0], [0], [4], 1, F32, BF16, source=[0], nsources=1)
    with pytest.raises(RuntimeError, match="DTYPE"):
        _lib.Runs([0], [0], [0], [4], 1, BF16, F32)


@pytest.mark.parametrize("bad", [torch.float16, torch.bfloat16, torch.float64, "float32"])
def test_state_refuses_other_residual_dtypes_before_the_device_check(bad):
    from powersgd_amd import Config
    from powersgd_amd.ddp import PowerSGDState

    p = torch.nn.Parameter(torch.zeros(4, 2, dtype=torch.bfloat16))  # a CPU tensor
    with pytest.raises(ValueError, match="residual_dtype"):
        PowerSGDState(Config(rank=1), [p], residual_dtype=bad)
    with pytest.raises(ValueError, match="residual_dtype"):  # fp32 residual over fp64 gradients
        PowerSGDState(Config(rank=1), [torch.nn.Parameter(torch.zeros(4, 2, dtype=torch.float64))],
                      residual_dtype=torch.float32)
