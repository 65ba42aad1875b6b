"""Host side of the IPC exchange for wide plans (psgd_ipc_create2, psgd_ipc_two_shot,
psgd_ipc_shard): the partition the two-shot kernels use, and the argument checks that need no
device. No GPU compute."""
import ctypes

import pytest

from powersgd_amd import _lib

NS = [0, 1, 3, 4, 5, 1369, 14650, 20569]
WORLDS = [1, 2, 3, 4, 8, 64]
VALUE = 2  # PSGD_ERR_VALUE


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("n", NS)
def test_shards_partition_the_factor(n, world):
    shards = [_lib.ipc_shard(n, world, r) for r in range(world)]
    per = 4 * (((n + 3) // 4 + world - 1) // world)  # floats per shard: whole quads
    pos = 0
    for begin, count in shards:
        assert begin % 4 == 0 and 0 <= count <= per
        if count:
            assert begin == pos  # contiguous, disjoint, in rank order
            pos = begin + count
            assert count == per or pos == n  # only the last non-empty shard is clipped
        else:
            assert pos == n  # empty shards come after the factor's end
    assert pos == n  # [0, n) is covered
    assert sum(c for _, c in shards) == n


def test_shard_argument_errors():
    L = _lib.lib()
    b, c = ctypes.c_int64(), ctypes.c_int64()
    assert L.psgd_ipc_shard(16, 2, 0, None, ctypes.byref(c)) == VALUE
    assert L.psgd_ipc_shard(16, 2, 0, ctypes.byref(b), None) == VALUE
    for world, rank in [(0, 0), (-1, 0), (65, 0), (2, 2), (2, -1), (64, 64)]:
        with pytest.raises(ValueError):
            _lib.ipc_shard(16, world, rank)
    with pytest.raises(ValueError):
        _lib.ipc_shard(-1, 2, 0)
    assert _lib.ipc_shard(16, 64, 63) == (16, 0)


def test_create2_argument_errors_need_no_device():
    L = _lib.lib()
    n = ctypes.c_int64()
    _lib.check(L.psgd_ipc_handle_bytes(ctypes.byref(n)))
    buf = (ctypes.c_uint8 * n.value)()
    plan = _lib.Plan([(300, 200), (200, 1000)], 64, 2, _lib.PSGD_F32)  # wide, unbound
    assert plan.is_wide()
    assert L.psgd_ipc_create2(None, 0, 2, buf) == VALUE
    assert L.psgd_ipc_create2(plan._h, 0, 2, None) == VALUE
    for mode in (3, -1):
        with pytest.raises(ValueError, match="mode"):
            plan.ipc_create2(0, mode)
    for mode in (0, 1, 2):  # the mode is checked before the plan's state
        with pytest.raises(RuntimeError, match="STATE.*not bound"):
            plan.ipc_create2(0, mode)
    narrow = _lib.Plan([(300, 200)], 4, 2, _lib.PSGD_F32)
    with pytest.raises(RuntimeError, match="STATE.*not bound"):
        narrow.ipc_create2(0, 1)
    # the old entry keeps its contract for either plan
    with pytest.raises(RuntimeError, match="STATE.*not bound"):
        plan.ipc_create(0)


def test_two_shot_query_arguments():
    L = _lib.lib()
    plan = _lib.Plan([(300, 200)], 64, 2, _lib.PSGD_F32)
    out = ctypes.c_int32()
    assert L.psgd_ipc_two_shot(None, 0, ctypes.byref(out)) == VALUE
    assert L.psgd_ipc_two_shot(plan._h, 0, None) == VALUE
    with pytest.raises(ValueError, match="side"):
        plan.ipc_two_shot(2)
    with pytest.raises(RuntimeError, match="STATE.*psgd_ipc_open first"):
        plan.ipc_two_shot(0)


def test_bindings_exist():
    L = _lib.lib()
    for name in ("psgd_ipc_create2", "psgd_ipc_two_shot", "psgd_ipc_shard"):
        assert name in _lib._SIGNATURES and getattr(L, name).restype is ctypes.c_int32
    assert callable(_lib.Plan.ipc_create2) and callable(_lib.Plan.ipc_two_shot) and callable(_lib.ipc_shard)
