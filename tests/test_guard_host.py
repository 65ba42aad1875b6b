"""Host-side contract of psgd_guard_outputs (include/psgd.h) and of the ``skip_nonfinite`` keyword
of ``PowerSGD``, ``Fp32ResidualPowerSGD`` and ``PowerSGDState``: what needs no device. The ctypes
signature against the header's prototype, the refusals that come before any device work (on an
unbound plan, so nothing can be launched), and the keyword's place in the three constructors."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from powersgd_amd import Config, Fp32ResidualPowerSGD, PowerSGD, _lib
from powersgd_amd.ddp import PowerSGDState

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3)]
ERR_VALUE, ERR_LAYOUT, ERR_STATE = 2, 4, 6

_CTYPE = {"psgd_plan*": ctypes.c_void_p, "void* const*": ctypes.c_void_p, "void*": ctypes.c_void_p,
          "const void*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64}


def _prototype(name):
    """Argument ctypes of `name` as include/psgd.h declares it."""
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
    assert m, name
    args = []
    for a in m.group(1).replace("\n", " ").split(","):
        words = a.split()
        args.append(_CTYPE[" ".join(words[:-1])])  # drop the parameter's name
    return args


def test_signature_table_matches_header():
    name = "psgd_guard_outputs"
    assert name in _lib.EXPORTED_SYMBOLS
    getattr(_lib.lib(), name)
    args, res = _lib._SIGNATURES[name]
    assert res is ctypes.c_int32
    assert args == _prototype(name)
    assert len(args) == 9
    assert callable(_lib.Plan.guard_outputs)
    with open(os.path.join(REPO, "include", "psgd.h")) as f:
        header = f.read()
    assert header.index("int psgd_clip_outputs(") < header.index("int psgd_guard_outputs(")


@pytest.mark.parametrize("dtype", [_lib.PSGD_F32, _lib.PSGD_BF16, _lib.PSGD_F64])
def test_refusals_before_any_device_work(dtype):
    """An unbound plan: every refusal below is decided from the arguments alone, in the order value,
    layout, state."""
    plan = _lib.Plan(SHAPES, 4, 2, dtype)
    L = _lib.lib()
    esz = {_lib.PSGD_F32: 4, _lib.PSGD_BF16: 2, _lib.PSGD_F64: 8}[dtype]
    fesz = 8 if dtype == _lib.PSGD_F64 else 4
    grads = _lib.ptr_array([4096 * (i + 1) for i in range(len(SHAPES))])  # never dereferenced
    g = ctypes.addressof(grads)
    A, R = 1 << 20, 1 << 21  # aligned stand-in addresses

    def call(plan_h=plan._h, grads=g, out=A, flat=A, n=8, p=A, q=A, res=R):
        return L.psgd_guard_outputs(plan_h, grads, out, flat, n, p, q, res, None)

    # value
    assert call(plan_h=None) == ERR_VALUE
    assert call(res=None) == ERR_VALUE
    assert call(grads=None) == ERR_VALUE  # a compressing call
    assert call(p=None) == ERR_VALUE
    assert call(q=None) == ERR_VALUE
    assert call(flat=None, n=8) == ERR_VALUE
    assert call(n=-1) == ERR_VALUE
    null_entry = _lib.ptr_array([4096, 0, 4096, 4096])
    assert call(grads=ctypes.addressof(null_entry)) == ERR_VALUE
    # layout (the plan is still unbound: layout is refused first)
    assert call(res=R + 4) == ERR_LAYOUT
    if esz > 1:
        assert call(out=A + esz // 2) == ERR_LAYOUT
        assert call(flat=A + esz // 2) == ERR_LAYOUT
        odd = _lib.ptr_array([4096, 4096 + esz // 2, 4096, 4096])
        assert call(grads=ctypes.addressof(odd)) == ERR_LAYOUT
    assert call(p=A + fesz // 2) == ERR_LAYOUT
    assert call(q=A + fesz // 2) == ERR_LAYOUT
    # element alignment is all a buffer needs
    assert call(out=A + esz, flat=A + esz, p=A + fesz, q=A + fesz) == ERR_STATE
    # state: a warm-up call (no out: grads, p_init, q_init ignored) and a compressing one
    assert call(grads=None, out=None, p=None, q=None) == ERR_STATE
    assert call() == ERR_STATE
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.guard_outputs(g, A, A, 8, A, A, R, 0)
    with pytest.raises(ValueError, match="null argument"):
        plan.guard_outputs(g, A, A, 8, A, A, 0, 0)
    with pytest.raises(RuntimeError, match="LAYOUT"):
        plan.guard_outputs(g, A, A, 8, A, A, R + 4, 0)


def test_keyword_only_with_default_false():
    p = inspect.signature(PowerSGD.__init__).parameters["skip_nonfinite"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert isinstance(PowerSGD.skip_nonfinite, property)
    for cls in (Fp32ResidualPowerSGD, PowerSGDState):  # taken at the class call
        p = inspect.signature(type(cls).__call__).parameters["skip_nonfinite"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
        for name in ("skip_nonfinite", "last_step_skipped", "skipped_steps"):
            assert isinstance(getattr(cls, name), property), (cls, name)
    with pytest.raises(TypeError):
        PowerSGD([torch.zeros(8, 8)], Config(rank=1), None, True)  # positional


def test_init_parameter_lists_unchanged():
    assert list(inspect.signature(PowerSGD.__init__).parameters)[:3] == ["self", "params", "config"]
    assert list(inspect.signature(PowerSGD.__init__).parameters)[3:] == ["max_grad_norm", "skip_nonfinite"]
    p = inspect.signature(PowerSGD.__init__).parameters["max_grad_norm"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert list(inspect.signature(Fp32ResidualPowerSGD.__init__).parameters)[1:] == ["params", "config", "fused"]
    assert list(inspect.signature(PowerSGDState.__init__).parameters)[1:] == [
        "config", "params", "process_group", "residual_dtype", "fused"]


def test_setter_refuses_after_the_first_aggregate():
    agg = object.__new__(PowerSGD)  # the setter alone (a constructed aggregator needs a GPU)
    agg._skip_nonfinite = False
    agg.step_counter = 1
    with pytest.raises(ValueError, match="before the first aggregate"):
        agg.skip_nonfinite = True
    assert agg.skip_nonfinite is False
    agg.skip_nonfinite = False  # no change: accepted at any time
