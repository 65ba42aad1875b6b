"""Host-side contract of psgd_aggregate_mixed / psgd_plan_mixed_folds (include/psgd.h): what
needs no device. The fold query on unbound plans, the ctypes signature table, the refusals that
come before any device work, and the Python keyword's default."""
import ctypes
import inspect
import os
import re

import pytest

from powersgd_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3)]
NEW = ("psgd_aggregate_mixed", "psgd_aggregate_mixed_flat", "psgd_plan_mixed_folds")


@pytest.mark.parametrize("rank,iters,dtype", [(8, 2, _lib.PSGD_F32), (64, 1, _lib.PSGD_F32), (2, 2, _lib.PSGD_BF16),
                                              (1, 1, _lib.PSGD_BF16), (2, 2, _lib.PSGD_F64)])
def test_ineligible_plans_report_no_folds(rank, iters, dtype):
    plan = _lib.Plan(SHAPES, rank, iters, dtype)
    for step in range(4):
        assert plan.mixed_folds(step) == (0, 0)


@pytest.mark.parametrize("rank", [1, 2, 4])
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_eligible_unbound_plan_answers_without_a_device(rank, iters):
    """Admission is asked of the runtime: without a device nothing is admitted (0 / 0), with one
    the answer is this build's. Either way: flags, and no ingest fold without the output fold."""
    plan = _lib.Plan(SHAPES, rank, iters, _lib.PSGD_F32)
    for step in range(4):
        fi, fo = plan.mixed_folds(step)
        assert fi in (0, 1) and fo in (0, 1) and fi <= fo
    assert plan.mixed_folds(0)[1] == plan.mixed_folds(2)[1]  # a property of the step's parity


def test_fold_query_argument_errors():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    with pytest.raises(ValueError, match="step out of range"):
        plan.mixed_folds(-1)
    L = _lib.lib()
    fi = ctypes.c_int32()
    assert L.psgd_plan_mixed_folds(None, 0, ctypes.byref(fi), ctypes.byref(fi)) == 2
    assert L.psgd_plan_mixed_folds(plan._h, 0, None, ctypes.byref(fi)) == 2
    assert b"null argument" in L.psgd_last_error()


def test_signature_table_and_header():
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(_lib.lib(), name)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib._SIGNATURES["psgd_aggregate_mixed"] == ([vp, vp, vp, vp, i64, vp], ctypes.c_int32)
    assert _lib._SIGNATURES["psgd_aggregate_mixed_flat"] == ([vp, vp, vp, vp, i64, vp, vp, vp, vp, vp], ctypes.c_int32)
    args, res = _lib._SIGNATURES["psgd_plan_mixed_folds"]
    assert len(args) == 4 and args[:2] == [vp, i64] and res is ctypes.c_int32
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name


def test_refusals_before_any_device_work():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    addr = ctypes.addressof(ptrs)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed(None, addr, 16, 0, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed(addr, addr, None, 0, 0)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed(addr, addr, 16, 0, 0)
    flat = _lib.FlatPlan([40, 96], _lib.PSGD_F32)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed(addr, addr, 16, 0, 0, flat=flat, unc_bf16=addr, unc_residual=addr, flat_out=16)


def test_fused_keyword_defaults_to_off():
    from powersgd_amd import Fp32ResidualPowerSGD

    sig = inspect.signature(Fp32ResidualPowerSGD.__init__)
    assert list(sig.parameters)[1:] == ["params", "config", "fused"]
    assert sig.parameters["fused"].default is False
