"""Host-side contract of psgd_sgd_update_mp / psgd_aggregate_mixed_comm_sgd[_wide] and their queries
(include/psgd.h), and of sgd_master_step's pairing: refusal codes, which come before any device work."""
import ctypes
import os
import re

import pytest
import torch

import powersgd_amd
from powersgd_amd import _lib

ERR_VALUE, ERR_LAYOUT, ERR_STATE = 2, 4, 6  # psgd_status (include/psgd.h)
NEW = ("psgd_sgd_update_mp", "psgd_aggregate_mixed_comm_sgd", "psgd_plan_mixed_sgd_ok",
       "psgd_aggregate_mixed_comm_sgd_wide", "psgd_plan_mixed_sgd_wide_ok")
_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


def test_new_entries_are_declared_with_the_signatures_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M) and name in _lib.EXPORTED_SYMBOLS, name
    entry = ([_vp] * 7 + [_i64] + [_vp] * 8, _i32)
    query = ([_vp, _i64, _i32, _i32, ctypes.POINTER(_i32)], _i32)
    assert _lib._SIGNATURES[NEW[0]] == ([_vp, _i32] + [_vp] * 7, _i32)
    assert _lib._SIGNATURES[NEW[1]] == _lib._SIGNATURES[NEW[3]] == entry
    assert _lib._SIGNATURES[NEW[2]] == _lib._SIGNATURES[NEW[4]] == query


def test_sgd_update_mp_refusals_in_order():
    L, a = _lib.lib(), ctypes.addressof
    g, p, b, w = (_lib.ptr_array([x]) for x in (0x1000, 0x2000, 0x3000, 0x5000))  # never dereferenced
    n, h = (_i64 * 1)(8), _lib.sgd_hyper([(0.1, 0.9, 0.0, 0.0, False, False)])
    good = [a(g), a(p), a(b), a(w), a(n), a(h)]
    for k in (0, 1, 3, 4, 5):  # every null table but buf's, which is judged per record
        args = list(good)
        args[k] = None
        assert L.psgd_sgd_update_mp(None, 1, *args, None) == ERR_VALUE and b"null argument" in L.psgd_last_error()
    null, odd_w, odd_p = _lib.ptr_array([0]), _lib.ptr_array([0x5001]), _lib.ptr_array([0x2002])
    plan = _lib.Plan([(8, 8)], 1, 1, _lib.PSGD_F32)
    assert L.psgd_sgd_update_mp(plan._h, 1, a(g), a(p), a(b), a(null), a(n), a(h), None) == ERR_STATE  # unbound first
    assert L.psgd_sgd_update_mp(None, 1, a(g), a(p), a(b), a(null), a(n), a(h), None) == ERR_VALUE
    assert b"null bf16 model parameter" in L.psgd_last_error()
    assert L.psgd_sgd_update_mp(None, 1, a(g), a(p), a(null), a(odd_w), a(n), a(h), None) == ERR_VALUE
    assert b"null momentum buffer" in L.psgd_last_error()
    assert L.psgd_sgd_update_mp(None, 1, a(g), a(odd_p), a(b), a(odd_w), a(n), a(h), None) == ERR_LAYOUT
    assert b"4-byte aligned" in L.psgd_last_error()
    assert L.psgd_sgd_update_mp(None, 1, a(g), a(p), a(b), a(odd_w), a(n), a(h), None) == ERR_LAYOUT
    assert b"2-byte aligned" in L.psgd_last_error()


@pytest.mark.parametrize("wide", [False, True])
def test_entries_and_queries_refuse_before_the_device(wide):
    L, a = _lib.lib(), ctypes.addressof
    entry = L.psgd_aggregate_mixed_comm_sgd_wide if wide else L.psgd_aggregate_mixed_comm_sgd
    query = L.psgd_plan_mixed_sgd_wide_ok if wide else L.psgd_plan_mixed_sgd_ok
    tabs = [_lib.ptr_array([0x1000 * (k + 1)]) for k in range(5)]  # g16, residual, w16, masters, bufs
    h = _lib.sgd_hyper([(0.1, 0.9, 0.0, 0.0, False, False)])
    plan = _lib.Plan([(128, 128)], 64 if wide else 1, 1, _lib.PSGD_F32)
    good = [a(t) for t in tabs] + [a(h)]
    tail = (0, None, None, None, None, None, None, None, None)  # step, flat, unc x 5, comm, stream
    for k in (0, 1, 2, 3, 5):  # a null bufs table is judged per record, after the plan's state
        args = list(good)
        args[k] = None
        assert entry(plan._h, *args, *tail) == ERR_VALUE and b"null argument" in L.psgd_last_error()
    assert entry(plan._h, *good, *tail) == ERR_STATE and b"not bound" in L.psgd_last_error()
    ok = _i32(7)
    assert query(None, 0, 1, 1, ctypes.byref(ok)) == ERR_VALUE
    assert query(plan._h, -1, 1, 1, ctypes.byref(ok)) == ERR_VALUE
    assert query(plan._h, 0, 0, 1, ctypes.byref(ok)) == ERR_VALUE
    assert query(plan._h, 0, 1, 2, ctypes.byref(ok)) == ERR_VALUE
    # refused by shape, no device asked: fp64 and bf16 plans, and a wide plan on the narrow query and the reverse
    shapes = [(_lib.PSGD_F64, 1, 1), (_lib.PSGD_BF16, 1, 1), (_lib.PSGD_F32, 1 if wide else 64, 1)]
    for dtype, rank, iters in shapes + ([] if wide else [(_lib.PSGD_F32, 8, 2)]):  # and rank bucket 8 at I = 2
        other = _lib.Plan([(128, 128)], rank, iters, dtype)
        ok.value = 7
        assert query(other._h, 0, 1, 1, ctypes.byref(ok)) == 0 and ok.value == 0, (dtype, rank)


def test_model_params_must_pair_with_the_masters_one_to_one():
    masters = [torch.nn.Parameter(torch.zeros(4, 4)), torch.nn.Parameter(torch.zeros(3))]
    opt = torch.optim.SGD(masters, lr=0.1)
    for model in ([torch.zeros(4, 4, dtype=torch.bfloat16)], [torch.zeros(4, 4, dtype=torch.bfloat16), torch.zeros(4)]):
        for fn in (powersgd_amd.sgd_master_step, powersgd_amd.sgd_master_step_applies):
            with pytest.raises(ValueError, match="sgd_master_step: .* pair one to one"):
                fn(opt, object.__new__(powersgd_amd.Fp32ResidualPowerSGD), model)
