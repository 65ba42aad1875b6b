"""Host-side contract of psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst / psgd_plan_dst_ok
(include/psgd.h) and of ``PowerSGDState.direct_store``: what needs no device. The ctypes signature
table and the header, the query on plans the calls never serve, the argument errors and the
refusals that come before any device work, the constructor's unchanged parameter list and the
setter's checks."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from powersgd_amd import _lib
from powersgd_amd.ddp import PowerSGDState

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3)]
NEW = ("psgd_aggregate_comm_dst", "psgd_aggregate_ipc_dst", "psgd_plan_dst_ok")
WORLDS = (1, 2, 3, 8)


def test_signature_table_and_header():
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(_lib.lib(), name)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    # (plan, grads, dst, step, flat, unc, unc_dst, comm, stream)
    assert _lib._SIGNATURES["psgd_aggregate_comm_dst"] == ([vp, vp, vp, i64, vp, vp, vp, vp, vp], i32)
    # (plan, grads, dst, step, flat, unc, unc_dst, stream)
    assert _lib._SIGNATURES["psgd_aggregate_ipc_dst"] == ([vp, vp, vp, i64, vp, vp, vp, vp], i32)
    # (plan, step, world, ok)
    assert _lib._SIGNATURES["psgd_plan_dst_ok"] == ([vp, i64, i32, ctypes.POINTER(i32)], i32)
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    for method in ("aggregate_comm_dst", "aggregate_ipc_dst", "dst_ok"):
        assert callable(getattr(_lib.Plan, method))


@pytest.mark.parametrize("rank,iters,dtype", [(2, 2, _lib.PSGD_BF16), (1, 1, _lib.PSGD_BF16), (2, 2, _lib.PSGD_F64),
                                              (64, 1, _lib.PSGD_F32), (64, 2, _lib.PSGD_F32)])
def test_plans_never_served_report_zero(rank, iters, dtype):
    plan = _lib.Plan(SHAPES, rank, iters, dtype)
    for world in WORLDS:
        for step in range(4):
            assert plan.dst_ok(step, world) == 0


def test_query_argument_errors():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    for world in (0, -1):
        with pytest.raises(ValueError, match="world size"):
            plan.dst_ok(0, world)
    with pytest.raises(ValueError, match="step out of range"):
        plan.dst_ok(-1, 2)
    L = _lib.lib()
    ok = ctypes.c_int32()
    assert L.psgd_plan_dst_ok(None, 0, 2, ctypes.byref(ok)) == 2
    assert L.psgd_plan_dst_ok(plan._h, 0, 2, None) == 2
    assert b"null argument" in L.psgd_last_error()


class _NoComm:  # a non-null communicator handle that is never dereferenced before the refusal
    _h = ctypes.c_void_p(16)


def test_refusals_before_any_device_work():
    plan = _lib.Plan(SHAPES, 8, 2, _lib.PSGD_F32)
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    addr = ctypes.addressof(ptrs)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_comm_dst(None, addr, 0, _NoComm, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_comm_dst(addr, None, 0, _NoComm, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_comm_dst(addr, addr, 0, None, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_ipc_dst(None, addr, 0, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_ipc_dst(addr, None, 0, 0)
    with pytest.raises(ValueError, match="step out of range"):
        plan.aggregate_ipc_dst(addr, addr, -1, 0)
    # "plan is not bound" comes before any device work (and, with a communicator, before the
    # step's range check, as in psgd_aggregate_comm)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_comm_dst(addr, addr, 0, _NoComm, 0)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_comm_dst(addr, addr, -1, _NoComm, 0)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_ipc_dst(addr, addr, 0, 0)
    flat = _lib.FlatPlan([40, 96], _lib.PSGD_F32)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_comm_dst(addr, addr, 0, _NoComm, 0, flat=flat, unc=addr, unc_dst=addr)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_ipc_dst(addr, addr, 0, 0, flat=flat, unc=addr, unc_dst=addr)


def test_constructor_parameter_list_is_unchanged():
    params = list(inspect.signature(PowerSGDState.__init__).parameters.values())
    assert [p.name for p in params] == ["self", "config", "params", "process_group", "residual_dtype", "fused"]
    assert params[-1].default is False
    assert isinstance(PowerSGDState.direct_store, property)
    assert PowerSGDState._direct is False  # the default: the three-stage completion


def _bare_state(param_dtype, residual_dtype, fused):
    """What the setter reads of a state, without a device: the parameters' dtype, the residual's
    and ``fused`` (a constructed state needs a GPU)."""
    st = object.__new__(PowerSGDState)
    st.params = [torch.nn.Parameter(torch.zeros(8, 8, dtype=param_dtype))]
    st.residual = torch.zeros(64, dtype=residual_dtype)
    st.fused = fused
    return st


@pytest.mark.parametrize("param_dtype,residual_dtype,fused", [(torch.bfloat16, torch.bfloat16, False),
                                                              (torch.bfloat16, torch.float32, False),
                                                              (torch.bfloat16, torch.float32, True),
                                                              (torch.float64, torch.float64, False)])
def test_direct_store_setter_refuses(param_dtype, residual_dtype, fused):
    st = _bare_state(param_dtype, residual_dtype, fused)
    assert st.direct_store is False
    with pytest.raises(ValueError, match="direct_store needs float32 parameters"):
        st.direct_store = True
    assert st.direct_store is False
    st.direct_store = False  # turning it off is always allowed
