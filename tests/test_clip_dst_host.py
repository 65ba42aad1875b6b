"""Host-side contract of psgd_clip_dst / psgd_plan_clip_dst_ok (include/psgd.h) and of
``PowerSGDState(..., max_grad_norm=...)``: what needs no device. The ctypes signature table and the
header, the query on plans the call never serves, the refusals that come before any device work
with their status codes, and the keyword's validation at the class call."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from powersgd_amd import Config, _lib
from powersgd_amd.ddp import PowerSGDState

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3)]
NEW = ("psgd_clip_dst", "psgd_plan_clip_dst_ok")
ERR_VALUE, ERR_STATE = 2, 6  # psgd_status (include/psgd.h)


def test_signature_table_and_header():
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(_lib.lib(), name)
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    # (plan, step, world, dst, flat, unc_dst, max_norm, result, stream)
    assert _lib._SIGNATURES["psgd_clip_dst"] == ([vp, i64, i32, vp, vp, vp, dbl, vp, vp], i32)
    # (plan, ok)
    assert _lib._SIGNATURES["psgd_plan_clip_dst_ok"] == ([vp, ctypes.POINTER(i32)], i32)
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert header.index("int psgd_clip_outputs(") < header.index("int psgd_clip_dst(")
    for method in ("clip_dst", "clip_dst_ok"):
        assert callable(getattr(_lib.Plan, method))
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        names = dict(re.findall(r"(PSGD_ERR_[A-Z]+)\s*=\s*(\d+)", f.read()))
    assert int(names["PSGD_ERR_VALUE"]) == ERR_VALUE and int(names["PSGD_ERR_STATE"]) == ERR_STATE


@pytest.mark.parametrize("what,rank,iters,dtype", [("bf16", 2, 2, _lib.PSGD_BF16), ("fp64", 2, 2, _lib.PSGD_F64),
                                                   ("rank 64", 64, 1, _lib.PSGD_F32),
                                                   ("rank 32 x 3 iterations", 32, 3, _lib.PSGD_F32)])
def test_plans_never_served_report_zero(what, rank, iters, dtype):
    plan = _lib.Plan(SHAPES, rank, iters, dtype)
    assert plan.clip_dst_ok() == 0, what
    # ... and the call refuses such a plan before it looks at its binding
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    res = (ctypes.c_double * 2)()
    st = _lib.lib().psgd_clip_dst(plan._h, 0, 1, ctypes.addressof(ptrs), None, None, 1.0, ctypes.addressof(res), None)
    assert st == ERR_VALUE, what


def test_two_buckets_report_zero_one_bucket_reports_one():
    plan = _lib.Plan(SHAPES, 4, 2, _lib.PSGD_F32)
    assert plan.clip_dst_ok() == 1
    ng = len(plan.groups())
    assert ng >= 2
    plan.set_buckets([1, ng])
    assert plan.clip_dst_ok() == 0
    plan.set_buckets([ng])
    assert plan.clip_dst_ok() == 1
    for rank, iters in ((1, 1), (1, 2), (2, 2), (4, 3), (16, 2), (32, 2), (16, 4)):
        assert _lib.Plan(SHAPES, rank, iters, _lib.PSGD_F32).clip_dst_ok() == 1, (rank, iters)


def test_query_argument_errors():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    L = _lib.lib()
    ok = ctypes.c_int32()
    assert L.psgd_plan_clip_dst_ok(None, ctypes.byref(ok)) == ERR_VALUE
    assert L.psgd_plan_clip_dst_ok(plan._h, None) == ERR_VALUE
    assert b"null argument" in L.psgd_last_error()


def test_refusals_before_any_device_work():
    L = _lib.lib()
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    assert plan.clip_dst_ok() == 1
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    addr = ctypes.addressof(ptrs)
    res = (ctypes.c_double * 2)()
    raddr = ctypes.addressof(res)
    flat = _lib.FlatPlan([40, 96], _lib.PSGD_F32)
    # nulls
    assert L.psgd_clip_dst(None, 0, 1, addr, None, None, 1.0, raddr, None) == ERR_VALUE
    assert L.psgd_clip_dst(plan._h, 0, 1, None, None, None, 1.0, raddr, None) == ERR_VALUE
    assert L.psgd_clip_dst(plan._h, 0, 1, addr, None, None, 1.0, None, None) == ERR_VALUE
    assert L.psgd_clip_dst(plan._h, 0, 1, addr, flat._h, None, 1.0, raddr, None) == ERR_VALUE  # flat, no unc_dst
    null_entry = _lib.ptr_array([16, 0])
    assert L.psgd_clip_dst(plan._h, 0, 1, addr, flat._h, ctypes.addressof(null_entry), 1.0, raddr, None) == ERR_VALUE
    null_dst = _lib.ptr_array([16, 0, 16, 16])
    assert L.psgd_clip_dst(plan._h, 0, 1, ctypes.addressof(null_dst), None, None, 1.0, raddr, None) == ERR_VALUE
    # max_norm
    for bad in (0.0, -1.0, math.nan):
        assert L.psgd_clip_dst(plan._h, 0, 1, addr, None, None, bad, raddr, None) == ERR_VALUE, bad
        assert b"max_norm" in L.psgd_last_error()
    # an unbound plan, with and without a flat tail, clipping or measuring
    for f, u in ((None, None), (flat._h, ctypes.addressof(_lib.ptr_array([16, 16])))):
        for x in (1.0, math.inf):
            assert L.psgd_clip_dst(plan._h, 0, 1, addr, f, u, x, raddr, None) == ERR_STATE
            assert b"not bound" in L.psgd_last_error()
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.clip_dst(0, 1, addr, 1.0, raddr, 0)
    with pytest.raises(ValueError, match="max_norm must be positive"):
        plan.clip_dst(0, 1, addr, 0.0, raddr, 0)
    assert res[0] == 0.0 and res[1] == 0.0  # nothing was written


def test_state_keyword_is_validated_before_any_device_work():
    params = [torch.nn.Parameter(torch.zeros(8, 8))]  # on the host: a constructed state needs a GPU
    cfg = Config(rank=2, num_iters_per_step=2, start_compressing_after_num_steps=0)
    for bad in (0, 0.0, -1, -1.5, math.nan):
        with pytest.raises(ValueError, match="max_grad_norm must be a positive number or None"):
            PowerSGDState(cfg, params, max_grad_norm=bad)
    # keyword only: the positional parameter list is the one existing callers use
    assert [p.name for p in inspect.signature(PowerSGDState.__init__).parameters.values()] == [
        "self", "config", "params", "process_group", "residual_dtype", "fused"]
    with pytest.raises(TypeError):
        PowerSGDState(cfg, params, None, None, False, 1.0)
    for name in ("max_grad_norm", "last_grad_norm", "last_clip_coef"):
        assert isinstance(getattr(PowerSGDState, name), property), name
    assert PowerSGDState.max_grad_norm.fset is not None
    assert PowerSGDState.last_grad_norm.fset is None and PowerSGDState.last_clip_coef.fset is None
