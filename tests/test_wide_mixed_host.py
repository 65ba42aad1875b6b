"""Host-side contract of psgd_aggregate_mixed_wide / psgd_aggregate_mixed_wide_comm /
psgd_plan_mixed_wide_ok (include/psgd.h): what needs no device. The ctypes signature table, the
eligibility query on plans the entries refuse, and the refusals that come before any device work,
in their documented order."""
import ctypes
import os
import re

import pytest

from powersgd_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 200), (200, 1000), (64, 3, 3, 3)]
NEW = ("psgd_aggregate_mixed_wide", "psgd_aggregate_mixed_wide_comm", "psgd_plan_mixed_wide_ok")
WORLDS = (1, 2, 3, 8)
VALUE = 2  # PSGD_ERR_VALUE


def test_signature_table_and_header():
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(_lib.lib(), name).restype is ctypes.c_int32
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    pi32 = ctypes.POINTER(i32)
    # (plan, grads_bf16, residual, out_bf16, step, flat, unc_bf16, unc_residual, flat_out_bf16, stream)
    assert _lib._SIGNATURES["psgd_aggregate_mixed_wide"] == ([vp, vp, vp, vp, i64, vp, vp, vp, vp, vp], i32)
    # (..., flat_out_bf16, comm, stream)
    assert _lib._SIGNATURES["psgd_aggregate_mixed_wide_comm"] == ([vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp], i32)
    # (plan, world, ok)
    assert _lib._SIGNATURES["psgd_plan_mixed_wide_ok"] == ([vp, i32, pi32], i32)
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name


@pytest.mark.parametrize("rank,dtype", [(1, _lib.PSGD_F32), (4, _lib.PSGD_F32), (32, _lib.PSGD_F32),
                                        (64, _lib.PSGD_BF16), (128, _lib.PSGD_BF16), (2, _lib.PSGD_F64)])
def test_plans_the_entries_refuse_are_not_ok(rank, dtype):
    plan = _lib.Plan(SHAPES, rank, 2, dtype)
    assert dtype != _lib.PSGD_F32 or not plan.is_wide()
    for world in WORLDS:
        assert plan.mixed_wide_ok(world) == 0


@pytest.mark.parametrize("rank", [64, 128])
def test_unbound_wide_plan_answers_for_every_world_or_none(rank):
    """Admission is asked of the runtime: without a device nothing is admitted, with one the
    answer is this build's. Either way it is a property of the plan, not of the world size."""
    plan = _lib.Plan(SHAPES, rank, 2, _lib.PSGD_F32)
    assert plan.is_wide()
    answers = {plan.mixed_wide_ok(world) for world in WORLDS}
    assert answers in ({0}, {1})


def test_query_argument_errors():
    L = _lib.lib()
    ok = ctypes.c_int32()
    for rank in (4, 64):  # the world size is checked before the plan's eligibility
        plan = _lib.Plan(SHAPES, rank, 2, _lib.PSGD_F32)
        for world in (0, -1):
            with pytest.raises(ValueError, match="world size must be >= 1"):
                plan.mixed_wide_ok(world)
        assert L.psgd_plan_mixed_wide_ok(plan._h, 1, None) == VALUE
        assert b"null argument" in L.psgd_last_error()
    assert L.psgd_plan_mixed_wide_ok(None, 1, ctypes.byref(ok)) == VALUE
    assert b"null argument" in L.psgd_last_error()


class _NoComm:  # a non-null communicator handle that is never dereferenced before the refusal
    _h = ctypes.c_void_p(16)


@pytest.mark.parametrize("comm", [None, _NoComm], ids=["wide", "wide_comm"])
def test_refusals_before_any_device_work(comm):
    plan = _lib.Plan(SHAPES, 64, 2, _lib.PSGD_F32)
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    addr = ctypes.addressof(ptrs)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_wide(None, addr, 16, 0, 0, comm=comm)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_wide(addr, None, 16, 0, 0, comm=comm)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_wide(addr, addr, None, 0, 0, comm=comm)
    # "not bound" comes before the step's range check
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_wide(addr, addr, 16, -1, 0, comm=comm)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_wide(addr, addr, 16, 0, 0, comm=comm)
    flat = _lib.FlatPlan([40, 96], _lib.PSGD_F32)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_wide(addr, addr, 16, 0, 0, comm=comm, flat=flat, unc_bf16=addr, unc_residual=addr,
                                  flat_out=16)


def test_null_communicator_is_a_null_argument():
    plan = _lib.Plan(SHAPES, 64, 2, _lib.PSGD_F32)
    addr = ctypes.addressof(_lib.ptr_array([16] * len(SHAPES)))
    st = _lib.lib().psgd_aggregate_mixed_wide_comm(plan._h, addr, addr, 16, 0, None, None, None, None, None, 0)
    assert st == VALUE and b"null argument" in _lib.lib().psgd_last_error()


def test_narrow_entries_report_no_folds_on_a_wide_plan():
    """A wide plan belongs to the wide entries alone: every narrow fold query answers 0, and the
    narrow entry's own order of checks ("not bound" first) is unchanged by the plan being wide."""
    plan = _lib.Plan(SHAPES, 64, 2, _lib.PSGD_F32)
    for step in range(4):
        assert plan.mixed_folds(step) == (0, 0)
        assert plan.mixed_folds_comm(step, 2) == (0, 0)
        assert plan.mixed_folds_dst(step, 2) == 0
    addr = ctypes.addressof(_lib.ptr_array([16] * len(SHAPES)))
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed(addr, addr, 16, 0, 0)


@pytest.mark.gpu
def test_mixed_flat_still_refuses_a_bound_wide_plan_by_rank():
    """The rank refusal comes after "not bound", so it needs a bound plan (a device): nothing is
    launched, the message is psgd_aggregate_mixed's own, and the same plan is one the wide query serves."""
    import torch

    from powersgd_amd.powersgd import BasicConfig, BasicPowerSGD

    dev = torch.device("cuda:0")
    shapes = [s for s in SHAPES if len(s) == 2]
    codec = BasicPowerSGD([torch.zeros(s, device=dev) for s in shapes], BasicConfig(64, 2))
    plan = codec._plan
    assert plan.is_wide() and plan.mixed_wide_ok(1) == 1
    grads = [torch.ones(s, dtype=torch.bfloat16, device=dev) for s in shapes]
    resid = [torch.ones(s, device=dev) for s in shapes]
    out = torch.zeros(sum(g.numel() for g in grads), dtype=torch.bfloat16, device=dev)
    flat = torch.zeros(8, dtype=torch.bfloat16, device=dev)
    gp = _lib.ptr_array([g.data_ptr() for g in grads])
    rp = _lib.ptr_array([r.data_ptr() for r in resid])
    stream = torch.cuda.current_stream(dev).cuda_stream
    msg = "psgd_aggregate_mixed serves rank buckets 1, 2, 4, 16 and 32"
    with pytest.raises(ValueError, match=msg):
        plan.aggregate_mixed(ctypes.addressof(gp), ctypes.addressof(rp), out.data_ptr(), 0, stream)
    st = _lib.lib().psgd_aggregate_mixed_flat(plan._h, gp, rp, out.data_ptr(), 0, None, None, None, flat.data_ptr(), stream)
    assert st == VALUE and msg.encode() in _lib.lib().psgd_last_error()
    torch.cuda.synchronize()
    assert all(bool((g == 1).all()) for g in grads) and all(bool((r == 1).all()) for r in resid)
    assert bool((out == 0).all())
