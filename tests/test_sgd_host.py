"""Host-side contract of psgd_sgd_update / psgd_aggregate_comm_sgd / psgd_plan_sgd_ok (include/psgd.h):
the refusal codes and their order, which come before any device work and so need no device."""
import ctypes

from powersgd_amd import _lib

ERR_VALUE, ERR_LAYOUT, ERR_STATE = 2, 4, 6  # psgd_status (include/psgd.h)


def _tables(p_addr=0x2000):
    """Host tables of one 8-element tensor at made-up device addresses (never dereferenced)."""
    return (_lib.ptr_array([0x1000]), _lib.ptr_array([p_addr]), _lib.ptr_array([0x3000]), (ctypes.c_int64 * 1)(8),
            _lib.sgd_hyper([(0.1, 0.9, 0.0, 0.0, False, False)]))


def test_sgd_update_refusals_in_order():
    L = _lib.lib()
    g, p, b, n, h = _tables()
    a = ctypes.addressof
    assert L.psgd_sgd_update(None, 1, None, a(p), a(b), a(n), a(h), None) == ERR_VALUE
    assert b"null argument" in L.psgd_last_error()
    assert L.psgd_sgd_update(None, 1, a(g), None, a(b), a(n), a(h), None) == ERR_VALUE
    assert L.psgd_sgd_update(None, 1, a(g), a(p), a(b), a(n), None, None) == ERR_VALUE
    assert L.psgd_sgd_update(None, 0, a(g), a(p), a(b), a(n), a(h), None) == ERR_VALUE
    # an unbound plan is refused after the null tables and before the entries are looked at
    plan = _lib.Plan([(8, 8)], 1, 1, _lib.PSGD_F32)
    _, bad_p, _, _, _ = _tables(0x2002)
    assert L.psgd_sgd_update(plan._h, 1, None, a(bad_p), a(b), a(n), a(h), None) == ERR_VALUE
    assert L.psgd_sgd_update(plan._h, 1, a(g), a(bad_p), a(b), a(n), a(h), None) == ERR_STATE
    assert b"not bound" in L.psgd_last_error()
    # no plan: a null momentum buffer of a tensor with momentum, then the misaligned p
    assert L.psgd_sgd_update(None, 1, a(g), a(bad_p), None, a(n), a(h), None) == ERR_VALUE
    assert b"momentum buffer" in L.psgd_last_error()
    assert L.psgd_sgd_update(None, 1, a(g), a(bad_p), a(b), a(n), a(h), None) == ERR_LAYOUT
    assert b"4-byte aligned" in L.psgd_last_error()


def test_aggregate_comm_sgd_and_query_refuse_before_the_device():
    L = _lib.lib()
    g, p, b, _, h = _tables()
    a = ctypes.addressof
    plan = _lib.Plan([(8, 8)], 1, 1, _lib.PSGD_F32)
    args = lambda gg, pp, hh: (plan._h, gg, pp, a(b), hh, 0, None, None, None, None, None, None)  # noqa: E731
    for gg, pp, hh in ((None, a(p), a(h)), (a(g), None, a(h)), (a(g), a(p), None)):
        assert L.psgd_aggregate_comm_sgd(*args(gg, pp, hh)) == ERR_VALUE
        assert b"null argument" in L.psgd_last_error()
    assert L.psgd_aggregate_comm_sgd(*args(a(g), a(p), a(h))) == ERR_STATE  # unbound, a null communicator is allowed
    assert b"not bound" in L.psgd_last_error()
    ok = ctypes.c_int32(7)
    assert L.psgd_plan_sgd_ok(None, 0, 1, 1, ctypes.byref(ok)) == ERR_VALUE
    assert L.psgd_plan_sgd_ok(plan._h, -1, 1, 1, ctypes.byref(ok)) == ERR_VALUE
    assert L.psgd_plan_sgd_ok(plan._h, 0, 0, 1, ctypes.byref(ok)) == ERR_VALUE
    assert L.psgd_plan_sgd_ok(plan._h, 0, 1, 2, ctypes.byref(ok)) == ERR_VALUE
    for dtype, rank in ((_lib.PSGD_BF16, 1), (_lib.PSGD_F64, 1), (_lib.PSGD_F32, 64)):  # refused by shape: no device asked
        other = _lib.Plan([(128, 128)], rank, 1, dtype)
        assert L.psgd_plan_sgd_ok(other._h, 0, 1, 1, ctypes.byref(ok)) == 0 and ok.value == 0
