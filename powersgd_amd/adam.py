"""``adam_step(optimizer, aggregator)``: ``optimizer_step`` for ``torch.optim.Adam`` / ``AdamW`` with the
optimizer's pass folded into the codec's final pass (psgd_aggregate_comm_adam, include/psgd.h).

``optimizer_step`` writes every average out as dense fp32, and the optimizer then reads it back with
the weight and both moments and writes all three. Here the final pass of the codec, at the element
where it would have stored the average, applies torch's single-tensor Adam rule to the weight,
``exp_avg`` and ``exp_avg_sq``: the averages never exist in memory and no optimizer launch follows.

Same contract as ``optimizer_step`` and ``sgd_step``: afterwards ``p.grad`` holds the error-feedback
buffer, the optimizer's state dict is torch's own (``exp_avg`` / ``exp_avg_sq`` created zero-filled
where absent; ``step`` torch's CPU scalar tensor, incremented by one per call and never moved to the
device) and the parameters have taken one step. The update rounds every operation to fp32 on its
own; torch's kernels may contract, so the two agree to rounding, not bit for bit.

The one-call form is taken when ``adam_step_applies`` says so; every other call IS
``optimizer_step(optimizer, aggregator)``. Both share the state dict, so warm-up steps and fused and
unfused steps mix freely. Hyperparameters, betas and the step count are read on every call, so a
scheduler may change ``lr`` between calls."""
from __future__ import annotations

from typing import List

import torch
from torch.optim.optimizer import _get_scalar_dtype

from . import _lib
from .powersgd import Aggregator, PowerSGD, _psgd_host, _stream
from .sgd import _comm_or_none
from .utils import params_in_optimizer


def _options_served(optimizer: torch.optim.Optimizer) -> bool:
    """Exactly ``torch.optim.Adam`` / ``AdamW`` with the options THE UPDATE covers and Python-number
    hyperparameters."""
    if type(optimizer) not in (torch.optim.Adam, torch.optim.AdamW):
        return False
    for g in optimizer.param_groups:
        if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable") or g.get("fused"):
            return False
        if any(torch.is_tensor(g[k]) for k in ("lr", "eps", "weight_decay")) or any(map(torch.is_tensor, g["betas"])):
            return False
    return True


def adam_step_applies(optimizer: torch.optim.Optimizer, aggregator: Aggregator) -> bool:
    """The NEXT ``adam_step`` takes the one-call form: exactly ``torch.optim.Adam`` or ``AdamW`` with
    ``amsgrad``, ``maximize``, ``capturable`` and ``differentiable`` off and ``fused`` not on, fp32
    contiguous parameters on the aggregator's device with gradients, a ``PowerSGD`` on a compressing
    step with neither ``max_grad_norm`` nor ``skip_nonfinite``, a process group over the library's
    communicator, and a plan psgd_plan_adam_ok (ranks 33-128: psgd_plan_adam_wide_ok) serves at both parities. Like ``sgd_step_applies`` it is
    a collective on its first compressing call (it creates the library's communicator)."""
    if not _options_served(optimizer) or type(aggregator) is not PowerSGD:
        return False
    params = params_in_optimizer(optimizer)
    dev = aggregator.device
    if not params or any(p.dtype != torch.float32 or p.device != dev or not p.is_contiguous() or p.grad is None
                         for p in params):
        return False
    if aggregator._powersgd.dtype != torch.float32 or len(params) != len(aggregator.is_compressed_mask):
        return False
    if aggregator.max_grad_norm is not None or aggregator.skip_nonfinite:
        return False
    if aggregator.step_counter + 1 <= aggregator.config.start_compressing_after_num_steps:
        return False
    comm = _comm_or_none(aggregator)
    if comm is None:
        return False
    plan = aggregator._powersgd._plan
    ok = plan.adam_wide_ok if plan.is_wide() else plan.adam_ok  # ranks 33-128: psgd_aggregate_comm_adam_wide
    return ok(0, comm.world) == 1 and ok(1, comm.world) == 1


def _records(optimizer: torch.optim.Optimizer, params: List[torch.Tensor]):
    """Per parameter the ``_lib.adam_hyper`` tuple and its two moments; creates absent state as torch's
    ``_init_group`` does and increments ``state["step"]``."""
    recs, ms, vs = {}, {}, {}
    adamw = type(optimizer) is torch.optim.AdamW
    for group in optimizer.param_groups:
        b1, b2 = (float(b) for b in group["betas"])
        decoupled = adamw or bool(group.get("decoupled_weight_decay", False))
        for p in group["params"]:
            state = optimizer.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["step"] += 1
            recs[p] = (float(group["lr"]), b1, b2, float(group["eps"]), float(group["weight_decay"]), decoupled,
                       float(state["step"]))
            ms[p], vs[p] = state["exp_avg"], state["exp_avg_sq"]
    return [recs[p] for p in params], [ms[p] for p in params], [vs[p] for p in params]


def adam_step(optimizer: torch.optim.Optimizer, aggregator: Aggregator) -> None:
    """Aggregate the gradients with ``aggregator`` and take the Adam / AdamW step with the aggregate, as
    ``optimizer_step`` (module docstring); in one library call where ``adam_step_applies``."""
    if not adam_step_applies(optimizer, aggregator):
        from . import optimizer_step

        return optimizer_step(optimizer, aggregator)
    params = params_in_optimizer(optimizer)
    grads = [p.grad.data for p in params]
    recs, ms, vs = _records(optimizer, params)
    mask = aggregator.is_compressed_mask
    codec = aggregator._powersgd
    tabs = getattr(aggregator, "_adam_tables", None)
    if tabs is None:
        shapes = [list(p.shape) for p in params]
        tabs = aggregator._adam_tables = tuple(_psgd_host.PtrTable(shapes, mask, _lib.PSGD_F32, codec._dev_index)
                                                for _ in range(3))
    ptab, mtab, vtab = tabs
    ptab.fill([p.data for p in params])
    mtab.fill(ms)
    vtab.fill(vs)
    # the records in the tables' order: the compressed tensors, then the uncompressed ones
    hyper = _lib.adam_hyper([r for r, c in zip(recs, mask) if c] + [r for r, c in zip(recs, mask) if not c])
    comm = _comm_or_none(aggregator)
    aggregator.step_counter += 1
    aggregator._table.fill(grads)
    kw = {}
    if aggregator._unc is not None:
        kw = dict(flat=aggregator._unc.plan, unc=aggregator._table.unc_addr(), unc_params=ptab.unc_addr(),
                  unc_ms=mtab.unc_addr(), unc_vs=vtab.unc_addr())
    codec._plan.aggregate_comm_adam(aggregator._table.comp_addr(), ptab.comp_addr(), mtab.comp_addr(), vtab.comp_addr(),
                                    hyper, codec.step_counter, comm, _stream(aggregator.device),
                                    wide=codec._plan.is_wide(), **kw)
    codec.step_counter += 1
