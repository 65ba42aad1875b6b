"""Host-side contract of psgd_aggregate_mixed_ipc / psgd_aggregate_mixed_ipc_dst (include/psgd.h):
what needs no device. The ctypes signature table, the header, the refusals that come before any
device work, and the routing of the bindings' optional flat arguments."""
import ctypes
import os
import re

import pytest

from powersgd_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3)]
NEW = ("psgd_aggregate_mixed_ipc", "psgd_aggregate_mixed_ipc_dst")
ERR_VALUE, ERR_STATE = 2, 6  # PSGD_ERR_VALUE, PSGD_ERR_STATE (include/psgd.h)


def test_signature_table_and_header():
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(_lib.lib(), name)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    # (plan, grads_bf16, residual, out_bf16, step, flat, unc_bf16, unc_residual, flat_out_bf16, stream)
    assert _lib._SIGNATURES["psgd_aggregate_mixed_ipc"] == ([vp, vp, vp, vp, i64, vp, vp, vp, vp, vp], i32)
    # (plan, residual, dst_bf16, step, flat, unc_residual, unc_dst_bf16, stream)
    assert _lib._SIGNATURES["psgd_aggregate_mixed_ipc_dst"] == ([vp, vp, vp, i64, vp, vp, vp, vp], i32)
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name


def test_status_codes_of_the_raw_entries():
    """Null arguments: PSGD_ERR_VALUE; step < 0: PSGD_ERR_VALUE (an argument error: it comes before
    the plan's state); an unbound plan: PSGD_ERR_STATE."""
    L = _lib.lib()
    assert _lib._STATUS_NAMES[ERR_VALUE] == "VALUE" and _lib._STATUS_NAMES[ERR_STATE] == "STATE"
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    a = ctypes.addressof(ptrs)
    dense, dst = L.psgd_aggregate_mixed_ipc, L.psgd_aggregate_mixed_ipc_dst
    assert dense(None, a, a, 16, 0, None, None, None, None, None) == ERR_VALUE
    assert dense(plan._h, None, a, 16, 0, None, None, None, None, None) == ERR_VALUE
    assert dense(plan._h, a, None, 16, 0, None, None, None, None, None) == ERR_VALUE
    assert dense(plan._h, a, a, None, 0, None, None, None, None, None) == ERR_VALUE
    assert b"null argument" in L.psgd_last_error()
    assert dst(None, a, a, 0, None, None, None, None) == ERR_VALUE
    assert dst(plan._h, None, a, 0, None, None, None, None) == ERR_VALUE
    assert dst(plan._h, a, None, 0, None, None, None, None) == ERR_VALUE
    assert b"null argument" in L.psgd_last_error()
    assert dense(plan._h, a, a, 16, 0, None, None, None, None, None) == ERR_STATE
    assert b"plan is not bound" in L.psgd_last_error()
    assert dst(plan._h, a, a, 0, None, None, None, None) == ERR_STATE
    assert b"plan is not bound" in L.psgd_last_error()
    assert dense(plan._h, a, a, 16, -1, None, None, None, None, None) == ERR_VALUE
    assert b"step out of range" in L.psgd_last_error()
    assert dst(plan._h, a, a, -1, None, None, None, None) == ERR_VALUE
    assert b"step out of range" in L.psgd_last_error()


def test_bindings_refuse_before_any_device_work():
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    ptrs = _lib.ptr_array([16] * len(SHAPES))
    addr = ctypes.addressof(ptrs)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_ipc(None, addr, 16, 0, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_ipc(addr, addr, None, 0, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_ipc_dst(None, addr, 0, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.aggregate_mixed_ipc_dst(addr, None, 0, 0)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_ipc(addr, addr, 16, 0, 0)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_ipc_dst(addr, addr, 0, 0)
    with pytest.raises(ValueError, match="step out of range"):
        plan.aggregate_mixed_ipc(addr, addr, 16, -1, 0)
    with pytest.raises(ValueError, match="step out of range"):
        plan.aggregate_mixed_ipc_dst(addr, addr, -1, 0)
    flat = _lib.FlatPlan([40, 96], _lib.PSGD_F32)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_ipc(addr, addr, 16, 0, 0, flat=flat, unc_bf16=addr, unc_residual=addr, flat_out=16)
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.aggregate_mixed_ipc_dst(addr, addr, 0, 0, flat=flat, unc_residual=addr, unc_dst_bf16=addr)


class _Spy:
    """Stands in for the loaded library: records the arguments of the one call made."""

    def __init__(self, name):
        self.name, self.args = name, None

    def __getattr__(self, name):
        assert name == self.name, name

        def call(*args):
            self.args = args
            return 0

        return call


def test_bindings_route_their_optional_flat_arguments(monkeypatch):
    """The bindings pass the flat plan's handle and the uncompressed tables in the C order; without
    a flat plan every flat argument is null (flat_out = 0 becomes a null pointer, not address 0)."""
    plan = _lib.Plan(SHAPES, 2, 2, _lib.PSGD_F32)
    flat = _lib.FlatPlan([40, 96], _lib.PSGD_F32)

    spy = _Spy("psgd_aggregate_mixed_ipc")
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    plan.aggregate_mixed_ipc(11, 12, 13, 5, 99)
    assert spy.args == (plan._h, 11, 12, 13, 5, None, None, None, None, 99)
    plan.aggregate_mixed_ipc(11, 12, 13, 5, 99, flat=flat, unc_bf16=21, unc_residual=22, flat_out=23)
    assert spy.args == (plan._h, 11, 12, 13, 5, flat._h, 21, 22, 23, 99)

    spy = _Spy("psgd_aggregate_mixed_ipc_dst")
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    plan.aggregate_mixed_ipc_dst(12, 14, 6, 98)
    assert spy.args == (plan._h, 12, 14, 6, None, None, None, 98)
    plan.aggregate_mixed_ipc_dst(12, 14, 6, 98, flat=flat, unc_residual=22, unc_dst_bf16=24)
    assert spy.args == (plan._h, 12, 14, 6, flat._h, 22, 24, 98)
    monkeypatch.undo()
