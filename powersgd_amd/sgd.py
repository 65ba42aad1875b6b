"""``sgd_step(optimizer, aggregator)``: ``optimizer_step`` for ``torch.optim.SGD`` with the optimizer's
pass folded into the codec's final pass (psgd_aggregate_comm_sgd, include/psgd.h).

``optimizer_step`` writes every average out as dense fp32, and ``torch.optim.SGD`` then reads it back
with the weight and the momentum buffer and writes both. Here the final pass of the codec, at the
element where it would have stored the average, applies the SGD update to the weight and the
momentum buffer: the averages never exist in memory and no optimizer launch follows. This is the
EF-SGD-with-momentum loop of the PowerSGD paper.

Same contract as ``optimizer_step``: afterwards ``p.grad`` holds the error-feedback buffer,
``optimizer.state[p]["momentum_buffer"]`` is torch's own buffer (created zero-filled on first use;
that step takes torch's ``buf = d`` rule for the tensor) and the parameters have taken one SGD
step. The update is torch's single-tensor rule with every multiply and add rounded to fp32 on its
own; torch's kernels may contract, so the two agree to rounding, not bit for bit.

The one-call form is taken when ``sgd_step_applies`` says so; every other call IS
``optimizer_step(optimizer, aggregator)``. Both share torch's state dict, so warm-up steps and later
steps mix freely. Hyperparameters are read from ``param_groups`` on every call."""
from __future__ import annotations

from typing import List

import torch

from . import _lib
from .powersgd import Aggregator, PowerSGD, _psgd_host, _stream
from .utils import is_distributed, params_in_optimizer


def _comm_or_none(aggregator: PowerSGD):
    """The library's communicator in a process group that runs over it, else None (not served).
    Outside a process group ``optimizer_step`` runs the world-size-1 step (the fused final kernels),
    whose residual rounds differently from the communicator sequence's: that case keeps
    ``optimizer_step``, so ``p.grad`` is bit for bit its residual wherever ``sgd_step`` is called."""
    codec = aggregator._powersgd
    if not is_distributed() or codec._ipc_mode():
        return None
    return codec._rccl_comm()


def _options_served(optimizer: torch.optim.Optimizer) -> bool:
    """Exactly ``torch.optim.SGD`` without ``maximize`` (THE UPDATE has no such form)."""
    if type(optimizer) is not torch.optim.SGD:
        return False
    return not any(g.get("maximize", False) for g in optimizer.param_groups)


def sgd_step_applies(optimizer: torch.optim.Optimizer, aggregator: Aggregator) -> bool:
    """The NEXT ``sgd_step`` takes the one-call form: a plain ``torch.optim.SGD`` without ``maximize``,
    fp32 contiguous parameters on one device, a ``PowerSGD`` on a compressing step with neither
    ``max_grad_norm`` nor ``skip_nonfinite`` (both act on averages that would no longer exist), a
    process group over the library's communicator, and a plan psgd_plan_sgd_ok (ranks 33-128:
    psgd_plan_sgd_wide_ok) serves.
    Not a pure query: the first call on a compressing step in a process group creates the library's
    communicator (``_rccl_comm``: a broadcast over the default group, a collective), so every rank
    calls it, or ``sgd_step``, at the same point, as ``PowerSGD.aggregate`` itself requires. The two
    plan queries are answered from the plan's admission cache after the first call."""
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
    ok = plan.sgd_wide_ok if plan.is_wide() else plan.sgd_ok  # ranks 33-128: psgd_aggregate_comm_sgd_wide
    return ok(0, comm.world) == 1 and ok(1, comm.world) == 1


def _records(optimizer: torch.optim.SGD, params: List[torch.Tensor]):
    """Per parameter (lr, momentum, dampening, weight_decay, nesterov, first) and its momentum
    buffer (torch's own; the parameter itself, never read, where the group has no momentum)."""
    recs, bufs = {}, {}
    for group in optimizer.param_groups:
        mu = float(group["momentum"])
        for p in group["params"]:
            first = False
            buf = p
            if mu != 0.0:
                state = optimizer.state[p]
                buf = state.get("momentum_buffer")
                if buf is None:
                    buf = state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    first = True
            recs[p] = (float(group["lr"]), mu, float(group["dampening"]), float(group["weight_decay"]),
                       bool(group["nesterov"]), first)
            bufs[p] = buf
    return [recs[p] for p in params], [bufs[p] for p in params]


def sgd_step(optimizer: torch.optim.Optimizer, aggregator: Aggregator) -> None:
    """Aggregate the gradients with ``aggregator`` and take the SGD step with the aggregate, as
    ``optimizer_step`` (module docstring); in one library call where ``sgd_step_applies``."""
    if not sgd_step_applies(optimizer, aggregator):
        from . import optimizer_step

        return optimizer_step(optimizer, aggregator)
    params = params_in_optimizer(optimizer)
    grads = [p.grad.data for p in params]
    recs, bufs = _records(optimizer, params)
    mask = aggregator.is_compressed_mask
    codec = aggregator._powersgd
    tabs = getattr(aggregator, "_sgd_tables", None)
    if tabs is None:
        shapes = [list(p.shape) for p in params]
        tabs = aggregator._sgd_tables = tuple(_psgd_host.PtrTable(shapes, mask, _lib.PSGD_F32, codec._dev_index)
                                               for _ in range(2))
    ptab, btab = tabs
    ptab.fill([p.data for p in params])
    btab.fill(bufs)
    # the records in the tables' order: the compressed tensors, then the uncompressed ones
    hyper = _lib.sgd_hyper([r for r, c in zip(recs, mask) if c] + [r for r, c in zip(recs, mask) if not c])
    comm = _comm_or_none(aggregator)
    aggregator.step_counter += 1
    aggregator._table.fill(grads)
    kw = {}
    if aggregator._unc is not None:
        kw = dict(flat=aggregator._unc.plan, unc=aggregator._table.unc_addr(), unc_params=ptab.unc_addr(),
                  unc_bufs=btab.unc_addr())
    codec._plan.aggregate_comm_sgd(aggregator._table.comp_addr(), ptab.comp_addr(), btab.comp_addr(), hyper,
                                   codec.step_counter, comm, _stream(aggregator.device), wide=codec._plan.is_wide(),
                                   **kw)
    codec.step_counter += 1
