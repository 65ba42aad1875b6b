"""``sgd_master_step(optimizer, aggregator, model_params)``: the SGD (momentum) step of a bf16 model whose
optimizer runs on fp32 master weights with fp32 momentum buffers, folded into the codec's final pass
(psgd_aggregate_mixed_comm_sgd, include/psgd.h). The mixed-precision form of ``sgd_step``, as
``adam_master_step`` is of ``adam_step``.

Unfused, the step stores the averages, ``optimizer.step()`` reads g, p and buf and writes p and buf,
and a copy reads p and writes the bf16 weight: about 30 bytes per element after the codec. Here the
bf16 gradients are added into the aggregator's fp32 residual (``Fp32ResidualPowerSGD``) and the final
pass of the codec, at the element where it would have stored the fp32 average, applies torch's
single-tensor SGD rule to the master weight and the momentum buffer, stores both and stores the new
weight rounded to bf16 at the model parameter's own address: 18 bytes per element with momentum, 10
without.

After the call the bf16 gradients are zero (consumed into the residual), the optimizer's state dict is
torch's own (``momentum_buffer`` created zero-filled on first use; that step takes torch's ``buf = d``
rule for the tensor), the masters have taken one step and every model parameter equals
``master.bfloat16()``.

The one-call form is taken when ``sgd_master_step_applies`` says so. Every other call runs
``adam_master``'s unfused sequence on the same state (``aggregate_fp32``, ``optimizer.step()``,
``model.copy_(master)``). Both forms feed the optimizer the same fp32 average, so they agree to the
update's own rounding and mix freely (warm-up steps)."""
from __future__ import annotations

from typing import Sequence

import torch

from . import _lib
from .adam_master import _paired, _unfused
from .powersgd import _psgd_host, _stream
from .residual import Fp32ResidualPowerSGD
from .sgd import _comm_or_none, _options_served, _records


def sgd_master_step_applies(optimizer: torch.optim.Optimizer, aggregator: Fp32ResidualPowerSGD,
                            model_params: Sequence[torch.Tensor]) -> bool:
    """The NEXT ``sgd_master_step`` takes the one-call form: the optimizer under ``sgd_step_applies``'s
    option rules (and no ``nesterov`` with ``dampening``, a pair torch's constructor refuses) over fp32
    contiguous masters, an ``Fp32ResidualPowerSGD`` over the bf16 contiguous ``model_params`` (with
    gradients) on its device, a compressing step with neither ``max_grad_norm`` nor ``skip_nonfinite``, a
    process group over the library's communicator, and a plan psgd_plan_mixed_sgd_ok (ranks 33-128:
    psgd_plan_mixed_sgd_wide_ok) serves at both parities. A collective on its first compressing call (it
    creates the library's communicator)."""
    if not _options_served(optimizer) or type(aggregator) is not Fp32ResidualPowerSGD:
        return False
    if any(g["nesterov"] and float(g["dampening"]) != 0.0 for g in optimizer.param_groups):
        return False
    masters, model = _paired(optimizer, model_params, "sgd_master_step")
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
    ok = plan.mixed_sgd_wide_ok if plan.is_wide() else plan.mixed_sgd_ok  # ranks 33-128: the wide entry
    return ok(0, comm.world) == 1 and ok(1, comm.world) == 1


def sgd_master_step(optimizer: torch.optim.Optimizer, aggregator: Fp32ResidualPowerSGD,
                    model_params: Sequence[torch.Tensor]) -> None:
    """Aggregate the bf16 gradients of ``model_params`` with ``aggregator``, take the SGD step on the
    optimizer's fp32 masters with the fp32 aggregate and refresh the bf16 model weights (module
    docstring); in one library call where ``sgd_master_step_applies``."""
    masters, model = _paired(optimizer, model_params, "sgd_master_step")
    if not sgd_master_step_applies(optimizer, aggregator, model):
        return _unfused(optimizer, aggregator, masters, model)
    inner, codec = aggregator.inner, aggregator.inner._powersgd
    mask = inner.is_compressed_mask
    recs, bufs = _records(optimizer, masters)
    tabs = getattr(aggregator, "_sgd_master_tables", None)
    if tabs is None:
        shapes = [list(p.shape) for p in masters]
        tabs = aggregator._sgd_master_tables = tuple(
            _psgd_host.PtrTable(shapes, mask, dt, aggregator._dev_index)
            for dt in (_lib.PSGD_BF16, _lib.PSGD_BF16, _lib.PSGD_F32, _lib.PSGD_F32))
    gtab, wtab, ptab, btab = tabs
    gtab.fill([w.grad.data for w in model])
    wtab.fill([w.data for w in model])
    ptab.fill([p.data for p in masters])
    btab.fill(bufs)
    # the records in the tables' order: the compressed tensors, then the uncompressed ones
    hyper = _lib.sgd_hyper([r for r, c in zip(recs, mask) if c] + [r for r, c in zip(recs, mask) if not c])
    comm = _comm_or_none(inner)
    inner._table.fill(aggregator.views)
    inner.step_counter += 1
    kw = {}
    if inner._unc is not None:
        kw = dict(flat=inner._unc.plan, unc_bf16=gtab.unc_addr(), unc_residual=inner._table.unc_addr(),
                  unc_params_bf16=wtab.unc_addr(), unc_masters=ptab.unc_addr(), unc_bufs=btab.unc_addr())
    codec._plan.aggregate_mixed_comm_sgd(gtab.comp_addr(), inner._table.comp_addr(), wtab.comp_addr(), ptab.comp_addr(),
                                         btab.comp_addr(), hyper, codec.step_counter, comm,
                                         _stream(aggregator.device), wide=codec._plan.is_wide(), **kw)
    codec.step_counter += 1
