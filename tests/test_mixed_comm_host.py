"""Host-side contract of psgd_aggregate_mixed_comm / psgd_plan_mixed_folds_comm (include/psgd.h):
what needs no device. The fold query on unbound plans, the ctypes signature table, and the
refusals that come before any device work."""
import ctypes
import os
import re

import pytest

from powersgd_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3)]
NEW = ("psgd_aggregate_mixed_comm", "psgd_plan_mixed_folds_comm")
WORLDS = (1, 2, 3, 8)


def test_signature_table_and_header():
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(_lib.lib(), name)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    pi32 = ctypes.POINTER(i32)
    # (plan, grads_bf16, residual, out_bf16, step, flat, unc_bf16, unc_residual, flat_out_bf16, comm, stream)
    assert _lib._SIGNATURES["psgd_aggregate_mixed_comm"] == ([vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp], i32)
    # (plan, step, world, fold_in, fold_out)
    assert _lib._SIGNATURES["psgd_plan_mixed_folds_comm"] == ([vp, i64, i32, pi32, pi32], i32)
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name


def test_version():
    assert _lib.lib().psgd_version() >= 102


@pytest.mark.parametrize("rank,iters,dtype", [(8, 2, _lib.PSGD_F32), (64, 1, _lib.PSGD_F32), (2, 2, _lib.PSGD_BF16),
                                              (1, 1, _lib.PSGD_BF16), (2, 2, _lib.PSGD_F64)])
def test_ineligible_plans_report_no_folds(rank, iters, dtype):
    plan = _lib.Plan(SHAPES, rank, iters, dtype)
    for world in WORLDS:
        for step in range(4):
            assert plan.mixed_folds_comm(step, world) == (0, 0)


def test_fold_query_argument_errors():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    for world in (0, -1):
        with pytest.raises(ValueError):
            plan.mixed_folds_comm(0, world)
    with pytest.raises(ValueError, match="step out of range"):
        plan.mixed_folds_comm(-1, 2)
    L = _lib.lib()
    fi = ctypes.c_int32()
    assert L.psgd_plan_mixed_folds_comm(None, 0, 2, ctypes.byref(fi), ctypes.byref(fi)) == 2
    assert L.psgd_plan_mixed_folds_comm(plan._h, 0, 2, None, ctypes.byref(fi)) == 2
    assert b"null argument" in L.psgd_last_error()


@pytest.mark.parametrize("rank", [1, 2, 4])
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_eligible_unbound_plan_never_folds_the_ingest(rank, iters):
    """Admission is asked of the runtime: without a device nothing is admitted (0 / 0), with one
    the answer is this build's. Either way the ingest is never folded in this form, and the output
    fold is a property of the plan, not of the step."""
    plan = _lib.Plan(SHAPES, rank, iters, _lib.PSGD_F32)
    for world in WORLDS:
        for step in range(4):
            fi, fo = plan.mixed_folds_comm(step, world)
            assert fi == 0 and fo in (0, 1)
        assert plan.mixed_folds_comm(0, world)[1] == plan.mixed_folds_comm(2, world)[1]


class _NoComm:  # a non-null communicator handle that is never dereferenced before the refusal
    _h = ctypes.c_void_p(16)


def test_refusals_before_any_device_work():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    addr = ctypes.addressof(ptrs)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_comm(None, addr, 16, 0, _NoComm, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_comm(addr, addr, None, 0, _NoComm, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_comm(addr, addr, 16, 0, None, 0)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_comm(addr, addr, 16, 0, _NoComm, 0)
    flat = _lib.FlatPlan([40, 96], _lib.PSGD_F32)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_comm(addr, addr, 16, 0, _NoComm, 0, flat=flat, unc_bf16=addr, unc_residual=addr,
                                  flat_out=16)
