"""Host-side contract of psgd_aggregate_mixed_comm_dst / psgd_plan_mixed_folds_dst (include/psgd.h)
and of ``PowerSGDState(..., fused=...)``: what needs no device. The ctypes signature table and the
header, the query on ineligible plans, the argument errors and the refusals that come before any
device work, the keyword's place, default and constructor checks."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from powersgd_amd import Config, _lib
from powersgd_amd.ddp import PowerSGDState

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3)]
NEW = ("psgd_aggregate_mixed_comm_dst", "psgd_plan_mixed_folds_dst")
WORLDS = (1, 2, 3, 8)


def test_signature_table_and_header():
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(_lib.lib(), name)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    # (plan, residual, dst_bf16, step, flat, unc_residual, unc_dst_bf16, comm, stream)
    assert _lib._SIGNATURES["psgd_aggregate_mixed_comm_dst"] == ([vp, vp, vp, i64, vp, vp, vp, vp, vp], i32)
    # (plan, step, world, fold_out)
    assert _lib._SIGNATURES["psgd_plan_mixed_folds_dst"] == ([vp, i64, i32, ctypes.POINTER(i32)], i32)
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name


@pytest.mark.parametrize("rank,iters,dtype", [(8, 2, _lib.PSGD_F32), (64, 1, _lib.PSGD_F32), (2, 2, _lib.PSGD_BF16),
                                              (1, 1, _lib.PSGD_BF16), (2, 2, _lib.PSGD_F64)])
def test_ineligible_plans_report_zero(rank, iters, dtype):
    plan = _lib.Plan(SHAPES, rank, iters, dtype)
    for world in WORLDS:
        for step in range(4):
            assert plan.mixed_folds_dst(step, world) == 0


@pytest.mark.parametrize("rank", [1, 2, 4])
def test_eligible_unbound_plan_answers_per_plan(rank):
    """Admission is asked of the runtime: without a device nothing is admitted, with one the
    answer is this build's; either way it is a property of the plan, not of the step."""
    plan = _lib.Plan(SHAPES, rank, 2, _lib.PSGD_F32)
    for world in WORLDS:
        assert plan.mixed_folds_dst(0, world) in (0, 1)
        assert plan.mixed_folds_dst(0, world) == plan.mixed_folds_dst(2, world)


def test_query_argument_errors():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    for world in (0, -1):
        with pytest.raises(ValueError, match="world size"):
            plan.mixed_folds_dst(0, world)
    with pytest.raises(ValueError, match="step out of range"):
        plan.mixed_folds_dst(-1, 2)
    L = _lib.lib()
    fo = ctypes.c_int32()
    assert L.psgd_plan_mixed_folds_dst(None, 0, 2, ctypes.byref(fo)) == 2
    assert L.psgd_plan_mixed_folds_dst(plan._h, 0, 2, None) == 2
    assert b"null argument" in L.psgd_last_error()


class _NoComm:  # a non-null communicator handle that is never dereferenced before the refusal
    _h = ctypes.c_void_p(16)


def test_refusals_before_any_device_work():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    addr = ctypes.addressof(ptrs)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_comm_dst(None, addr, 0, _NoComm, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_comm_dst(addr, None, 0, _NoComm, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_comm_dst(addr, addr, 0, None, 0)
    # "plan is not bound" comes before the step's range check and before any device work
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_comm_dst(addr, addr, 0, _NoComm, 0)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_comm_dst(addr, addr, -1, _NoComm, 0)
    flat = _lib.FlatPlan([40, 96], _lib.PSGD_F32)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_comm_dst(addr, addr, 0, _NoComm, 0, flat=flat, unc_residual=addr, unc_dst_bf16=addr)


def test_fused_keyword_is_last_and_defaults_to_false():
    params = list(inspect.signature(PowerSGDState.__init__).parameters.values())
    assert [p.name for p in params] == ["self", "config", "params", "process_group", "residual_dtype", "fused"]
    assert params[-1].default is False


@pytest.mark.parametrize("dtype,residual_dtype", [(torch.float32, torch.float32), (torch.float32, None),
                                                  (torch.bfloat16, None)])
def test_fused_needs_bf16_parameters_with_an_fp32_residual(dtype, residual_dtype):
    """Raised at construction, before the state looks at the device."""
    cfg = Config(rank=2, num_iters_per_step=2, start_compressing_after_num_steps=0)
    params = [torch.nn.Parameter(torch.zeros(8, 8, dtype=dtype))]
    with pytest.raises(ValueError, match="fused=True"):
        PowerSGDState(cfg, params, residual_dtype=residual_dtype, fused=True)
