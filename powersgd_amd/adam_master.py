"""``adam_master_step(optimizer, aggregator, model_params)``: the Adam / AdamW step of a bf16 model whose
optimizer runs on fp32 master weights with fp32 moments, folded into the codec's final pass
(psgd_aggregate_mixed_comm_adam, include/psgd.h).

Unfused, such a step is four element-wise passes over the whole model after the codec: the final
pass rounds and stores bf16 averages, a cast writes fp32 master gradients, the optimizer reads g, p,
m, v and writes p, m, v, and a copy writes the bf16 model weights. Here the bf16 gradients are added
into the aggregator's fp32 residual (``Fp32ResidualPowerSGD``) and the final pass of the codec, at
the element where it would have stored the fp32 average, applies torch's single-tensor Adam rule to
the master weight, ``exp_avg`` and ``exp_avg_sq``, stores all three and stores the new weight rounded
to bf16 at the model parameter's own address. No average, master gradient or copy pass exists.

After the call the bf16 gradients are zero (consumed into the residual, as ``aggregate`` leaves
them), the optimizer's state dict is torch's own (``step`` torch's CPU scalar, incremented by one),
the masters have taken one step and every model parameter equals ``master.bfloat16()``.

The one-call form is taken when ``adam_master_step_applies`` says so. Every other call runs the
unfused sequence on the same state: ``aggregator.aggregate_fp32`` (the ADD and the fp32 codec), the
unrounded fp32 averages as the masters' ``.grad`` for ``optimizer.step()`` (restored afterwards), and
``model.copy_(master)``. Both forms feed the optimizer the same fp32 average, so they agree to Adam's
own rounding, as ``adam_step`` and ``optimizer_step`` do, and mix freely (warm-up steps)."""
from __future__ import annotations

from typing import List, Sequence

import torch

from . import _lib
from .adam import _options_served, _records
from .powersgd import _psgd_host, _stream
from .residual import Fp32ResidualPowerSGD
from .sgd import _comm_or_none
from .utils import params_in_optimizer


def _paired(optimizer: torch.optim.Optimizer, model_params: Sequence[torch.Tensor], who: str = "adam_master_step"):
    masters = params_in_optimizer(optimizer)
    model = list(model_params)
    if len(masters) != len(model) or any(a.shape != b.shape for a, b in zip(masters, model)):
        raise ValueError(f"{who}: the optimizer's master parameters and model_params must pair one to one, "
                         "in order and shape")
    return masters, model


def adam_master_step_applies(optimizer: torch.optim.Optimizer, aggregator: Fp32ResidualPowerSGD,
                             model_params: Sequence[torch.Tensor]) -> bool:
    """The NEXT ``adam_master_step`` takes the one-call form: the optimizer under ``adam_step_applies``'s
    option rules over fp32 contiguous masters, an ``Fp32ResidualPowerSGD`` over the bf16 contiguous
    ``model_params`` (with gradients) on its device, a compressing step with neither ``max_grad_norm``
    nor ``skip_nonfinite``, a process group over the library's communicator, and a plan
    psgd_plan_mixed_adam_ok (ranks 33-128: psgd_plan_mixed_adam_wide_ok) serves at both parities. A collective on its first compressing call (it
    creates the library's communicator)."""
    if not _options_served(optimizer) or type(aggregator) is not Fp32ResidualPowerSGD:
        return False
    masters, model = _paired(optimizer, model_params)
    dev = aggregator.device
    if not masters or len(masters) != len(aggregator.is_compressed_mask):
        return False
    if any(p.dtype != torch.float32 or p.device != dev or not p.is_contiguous() for p in masters):
        return False
    if any(w.dtype != torch.bfloat16 or w.device != dev or not w.is_contiguous() or w.grad is None or
           w.shape != v.shape for w, v in zip(model, aggregator.views)):
        return False
    if aggregator.max_grad_norm is not None or aggregator.skip_nonfinite:
        return False
    if aggregator.step_counter + 1 <= aggregator.config.start_compressing_after_num_steps:
        return False
    comm = _comm_or_none(aggregator.inner)
    if comm is None:
        return False
    plan = aggregator.inner._powersgd._plan
    ok = plan.mixed_adam_wide_ok if plan.is_wide() else plan.mixed_adam_ok  # ranks 33-128: the wide entry
    return ok(0, comm.world) == 1 and ok(1, comm.world) == 1


def _unfused(optimizer, aggregator, masters: List[torch.Tensor], model: List[torch.Tensor]) -> None:
    avg = aggregator.aggregate_fp32([w.grad.data for w in model])
    saved = [p.grad for p in masters]
    for p, a in zip(masters, avg):
        p.grad = a
    optimizer.step()
    for p, g in zip(masters, saved):
        p.grad = g
    with torch.no_grad():
        torch._foreach_copy_([w.data for w in model], [p.data for p in masters])


def adam_master_step(optimizer: torch.optim.Optimizer, aggregator: Fp32ResidualPowerSGD,
                     model_params: Sequence[torch.Tensor]) -> None:
    """Aggregate the bf16 gradients of ``model_params`` with ``aggregator``, take the Adam / AdamW step
    on the optimizer's fp32 masters with the fp32 aggregate and refresh the bf16 model weights (module
    docstring); in one library call where ``adam_master_step_applies``."""
    masters, model = _paired(optimizer, model_params)
    if not adam_master_step_applies(optimizer, aggregator, model):
        return _unfused(optimizer, aggregator, masters, model)
    inner, codec = aggregator.inner, aggregator.inner._powersgd
    mask = inner.is_compressed_mask
    recs, ms, vs = _records(optimizer, masters)
    tabs = getattr(aggregator, "_adam_master_tables", None)
    if tabs is None:
        shapes = [list(p.shape) for p in masters]
        tabs = aggregator._adam_master_tables = tuple(
            _psgd_host.PtrTable(shapes, mask, dt, aggregator._dev_index)
            for dt in (_lib.PSGD_BF16, _lib.PSGD_BF16, _lib.PSGD_F32, _lib.PSGD_F32, _lib.PSGD_F32))
    gtab, wtab, ptab, mtab, vtab = tabs
    gtab.fill([w.grad.data for w in model])
    wtab.fill([w.data for w in model])
    ptab.fill([p.data for p in masters])
    mtab.fill(ms)
    vtab.fill(vs)
    # the records in the tables' order: the compressed tensors, then the uncompressed ones
    hyper = _lib.adam_hyper([r for r, c in zip(recs, mask) if c] + [r for r, c in zip(recs, mask) if not c])
    comm = _comm_or_none(inner)
    inner._table.fill(aggregator.views)
    inner.step_counter += 1
    kw = {}
    if inner._unc is not None:
        kw = dict(flat=inner._unc.plan, unc_bf16=gtab.unc_addr(), unc_residual=inner._table.unc_addr(),
                  unc_params_bf16=wtab.unc_addr(), unc_masters=ptab.unc_addr(), unc_ms=mtab.unc_addr(),
                  unc_vs=vtab.unc_addr())
    codec._plan.aggregate_mixed_comm_adam(gtab.comp_addr(), inner._table.comp_addr(), wtab.comp_addr(), ptab.comp_addr(),
                                          mtab.comp_addr(), vtab.comp_addr(), hyper, codec.step_counter, comm,
                                          _stream(aggregator.device), wide=codec._plan.is_wide(), **kw)
    codec.step_counter += 1
