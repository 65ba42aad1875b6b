"""Host-side contract of psgd_clip_outputs / psgd_plan_norm_form (include/psgd.h) and of
``PowerSGD(max_grad_norm=...)``: what needs no device. The ctypes signature table against the
header's prototypes, the form an unbound plan reports, the argument checks that come before any
device work, and the attribute's value checks."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from powersgd_amd import Config, PowerSGD, _lib
from powersgd_amd.residual import Fp32ResidualPowerSGD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 520), (300, 520), (130, 67), (64, 3, 3, 3)]
FACTORS, STREAM = _lib.Plan.NORM_FACTORS, _lib.Plan.NORM_STREAM

_CTYPE = {"psgd_plan*": ctypes.c_void_p, "const psgd_plan*": ctypes.c_void_p, "void*": ctypes.c_void_p,
          "double*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double,
          "int32_t*": ctypes.POINTER(ctypes.c_int32)}


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
    for name in ("psgd_clip_outputs", "psgd_plan_norm_form"):
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(_lib.lib(), name)
        args, res = _lib._SIGNATURES[name]
        assert res is ctypes.c_int32
        assert args == _prototype(name), name
    assert len(_lib._SIGNATURES["psgd_clip_outputs"][0]) == 10
    for method in ("clip_outputs", "norm_form"):
        assert callable(getattr(_lib.Plan, method))


@pytest.mark.parametrize("dtype", [_lib.PSGD_F32, _lib.PSGD_BF16])
@pytest.mark.parametrize("rank,iters", [(r, i) for r in (1, 2, 3, 4, 8, 16, 32) for i in (1, 2, 3, 4)])
def test_unbound_plan_form_by_rank_and_iterations(rank, iters, dtype, monkeypatch):
    monkeypatch.delenv("PSGD_NORM_FORM", raising=False)
    plan = _lib.Plan(SHAPES, rank, iters, dtype)
    bucket = 1
    while bucket < rank:
        bucket *= 2
    want = FACTORS if iters * bucket <= 64 else STREAM
    for step in (0, 1):
        for world in (1, 3):
            assert plan.norm_form(step, world) == want, (rank, iters)


def test_unbound_plan_stream_cases(monkeypatch):
    monkeypatch.delenv("PSGD_NORM_FORM", raising=False)
    assert _lib.Plan(SHAPES, 64, 1, _lib.PSGD_F32).norm_form(0, 1) == STREAM   # wide plan
    assert _lib.Plan(SHAPES, 4, 2, _lib.PSGD_F64).norm_form(0, 1) == STREAM    # fp64 factors
    assert _lib.Plan(SHAPES, 32, 3, _lib.PSGD_F32).norm_form(0, 1) == STREAM   # I x bucket = 96
    assert _lib.Plan(SHAPES, 32, 2, _lib.PSGD_F32).norm_form(0, 1) == FACTORS  # I x bucket = 64


def test_norm_form_environment_knob(monkeypatch):
    monkeypatch.setenv("PSGD_NORM_FORM", "stream")
    assert _lib.Plan(SHAPES, 4, 2, _lib.PSGD_F32).norm_form(0, 1) == STREAM
    monkeypatch.setenv("PSGD_NORM_FORM", "factors")
    assert _lib.Plan(SHAPES, 4, 2, _lib.PSGD_F32).norm_form(0, 1) == FACTORS
    assert _lib.Plan(SHAPES, 64, 2, _lib.PSGD_F32).norm_form(0, 1) == STREAM  # never where it does not apply
    monkeypatch.setenv("PSGD_NORM_FORM", "gram")
    with pytest.raises(ValueError, match="PSGD_NORM_FORM"):
        _lib.Plan(SHAPES, 4, 2, _lib.PSGD_F32)


def test_argument_errors_before_any_device_work():
    plan = _lib.Plan(SHAPES, 4, 2, _lib.PSGD_F32)
    with pytest.raises(ValueError, match="out of range"):
        plan.norm_form(-1, 1)
    with pytest.raises(ValueError, match="out of range"):
        plan.norm_form(0, 0)
    L = _lib.lib()
    f = ctypes.c_int32()
    assert L.psgd_plan_norm_form(None, 0, 1, ctypes.byref(f)) == 2
    assert L.psgd_plan_norm_form(plan._h, 0, 1, None) == 2
    with pytest.raises(ValueError, match="null argument"):
        plan.clip_outputs(0, 1, 16, 0, 0, 1.0, 0, 0)  # no result buffer
    with pytest.raises(RuntimeError, match="plan is not bound"):
        plan.clip_outputs(0, 1, 16, 0, 0, 1.0, 16, 0)


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1.5, float("nan")])
def test_bad_max_grad_norm_raises(bad):
    params = [torch.zeros(8, 8)]
    with pytest.raises(ValueError, match="max_grad_norm"):
        PowerSGD(params, Config(rank=1), max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        Fp32ResidualPowerSGD([torch.zeros(8, 8, dtype=torch.bfloat16)], Config(rank=1), max_grad_norm=bad)
    agg = object.__new__(PowerSGD)  # the setter alone (a constructed aggregator needs a GPU)
    agg._max_grad_norm = None
    with pytest.raises(ValueError, match="max_grad_norm"):
        agg.max_grad_norm = bad
    assert agg.max_grad_norm is None
    agg.max_grad_norm = 2
    assert agg.max_grad_norm == 2.0 and isinstance(agg.max_grad_norm, float)
    agg.max_grad_norm = math.inf  # the norm only
    agg.max_grad_norm = None


def test_keyword_only_and_defaults():
    p = inspect.signature(PowerSGD.__init__).parameters["max_grad_norm"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert [p for p in inspect.signature(PowerSGD.__init__).parameters][:3] == ["self", "params", "config"]
    # Fp32ResidualPowerSGD takes the keyword at the class call; __init__ keeps (params, config, fused)
    assert list(inspect.signature(Fp32ResidualPowerSGD.__init__).parameters)[1:] == ["params", "config", "fused"]
    with pytest.raises(TypeError):
        Fp32ResidualPowerSGD([torch.zeros(8, 8, dtype=torch.bfloat16)], Config(rank=1), False, 1.0)  # positional
    assert isinstance(Fp32ResidualPowerSGD.max_grad_norm, property)
