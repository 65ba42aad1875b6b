"""Host-side contract of psgd_adam_update / psgd_aggregate_comm_adam / psgd_plan_adam_ok (include/psgd.h)
and of adam_step's fall-back: refusal codes and their order, which come before any device work."""
import ctypes
import types

import pytest
import torch

import powersgd_amd
from powersgd_amd import _lib

ERR_VALUE, ERR_LAYOUT, ERR_STATE = 2, 4, 6  # psgd_status (include/psgd.h)
REC = (1e-3, 0.9, 0.999, 1e-8, 1e-2, True, 1.0)


def _tables(p_addr=0x2000):
    """Host tables of one 8-element tensor at made-up device addresses (never dereferenced)."""
    return (_lib.ptr_array([0x1000]), _lib.ptr_array([p_addr]), _lib.ptr_array([0x3000]), _lib.ptr_array([0x4000]),
            (ctypes.c_int64 * 1)(8), _lib.adam_hyper([REC]))


def test_adam_update_refusals_in_order():
    L = _lib.lib()
    a = ctypes.addressof
    g, p, m, v, n, h = _tables()
    good = [a(g), a(p), a(m), a(v), a(n), a(h)]
    for k in range(6):  # every null table
        args = list(good)
        args[k] = None
        assert L.psgd_adam_update(None, 1, *args, None) == ERR_VALUE
        assert b"null argument" in L.psgd_last_error()
    assert L.psgd_adam_update(None, 0, *good, None) == ERR_VALUE
    # an unbound plan is refused after the null tables and before the entries are looked at
    plan = _lib.Plan([(8, 8)], 1, 1, _lib.PSGD_F32)
    bad_p, null_v = _tables(0x2002)[1], _lib.ptr_array([0])
    assert L.psgd_adam_update(plan._h, 1, a(g), a(bad_p), a(m), a(null_v), a(n), a(h), None) == ERR_STATE
    assert b"not bound" in L.psgd_last_error()
    # no plan: a null moment, then the misaligned p
    assert L.psgd_adam_update(None, 1, a(g), a(bad_p), a(m), a(null_v), a(n), a(h), None) == ERR_VALUE
    assert b"null moment" in L.psgd_last_error()
    assert L.psgd_adam_update(None, 1, a(g), a(bad_p), a(m), a(v), a(n), a(h), None) == ERR_LAYOUT
    assert b"4-byte aligned" in L.psgd_last_error()


def test_aggregate_comm_adam_and_query_refuse_before_the_device():
    L = _lib.lib()
    a = ctypes.addressof
    g, p, m, v, _, h = _tables()
    plan = _lib.Plan([(8, 8)], 1, 1, _lib.PSGD_F32)
    good = [a(g), a(p), a(m), a(v), a(h)]
    tail = (0, None, None, None, None, None, None, None)  # step, flat, unc x 4, comm, stream
    for k in range(5):
        args = list(good)
        args[k] = None
        assert L.psgd_aggregate_comm_adam(plan._h, *args, *tail) == ERR_VALUE
        assert b"null argument" in L.psgd_last_error()
    assert L.psgd_aggregate_comm_adam(plan._h, *good, *tail) == ERR_STATE  # unbound; a null communicator is allowed
    assert b"not bound" in L.psgd_last_error()
    ok = ctypes.c_int32(7)
    assert L.psgd_plan_adam_ok(None, 0, 1, ctypes.byref(ok)) == ERR_VALUE
    assert L.psgd_plan_adam_ok(plan._h, -1, 1, ctypes.byref(ok)) == ERR_VALUE
    assert L.psgd_plan_adam_ok(plan._h, 0, 0, ctypes.byref(ok)) == ERR_VALUE
    for dtype, rank in ((_lib.PSGD_BF16, 1), (_lib.PSGD_F64, 1), (_lib.PSGD_F32, 64)):  # refused by shape: no device asked
        other = _lib.Plan([(128, 128)], rank, 1, dtype)
        assert L.psgd_plan_adam_ok(other._h, 0, 1, ctypes.byref(ok)) == 0 and ok.value == 0


def test_adam_hyper_is_torchs_double_arithmetic_rounded_once():
    h = _lib.adam_hyper([(1e-3, 0.9, 0.999, 1e-8, 1e-2, False, 3.0)])[0]
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    assert (h.w1, h.beta2, h.w2, h.eps) == (f32(1 - 0.9), f32(0.999), f32(1 - 0.999), f32(1e-8))
    assert (h.step_size, h.bc2_sqrt) == (f32(1e-3 / (1 - 0.9 ** 3.0)), f32((1 - 0.999 ** 3.0) ** 0.5))
    assert (h.weight_decay, h.decay, h.decoupled) == (f32(1e-2), f32(1 - 1e-3 * 1e-2), 0)


@pytest.mark.parametrize("case", ["amsgrad", "maximize", "capturable", "bf16", "sgd", "max_grad_norm"])
def test_adam_step_is_optimizer_step_where_it_does_not_apply(case, monkeypatch):
    """Each refusal is decided on the host before the plan is asked; adam_step then IS optimizer_step."""
    p = torch.nn.Parameter(torch.zeros(4, 4, dtype=torch.bfloat16 if case == "bf16" else torch.float32))
    p.grad = torch.zeros_like(p)
    kw = {case: True} if case in ("amsgrad", "maximize", "capturable") else {}
    opt = torch.optim.SGD([p], lr=0.1) if case == "sgd" else torch.optim.AdamW([p], lr=1e-3, **kw)
    agg = object.__new__(powersgd_amd.PowerSGD)  # the fields adam_step_applies reads before any device work
    agg.device, agg.is_compressed_mask, agg._skip_nonfinite = p.device, [True], False
    agg.max_grad_norm = 1.0 if case == "max_grad_norm" else None
    agg._powersgd = types.SimpleNamespace(dtype=p.dtype)
    calls = []
    monkeypatch.setattr(powersgd_amd, "optimizer_step", lambda *a: calls.append(a))
    assert not powersgd_amd.adam_step_applies(opt, agg)
    powersgd_amd.adam_step(opt, agg)
    assert calls == [(opt, agg)] and not opt.state[p]
