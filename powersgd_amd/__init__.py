"""powersgd_amd — MI355X-native PowerSGD gradient compression.

Drop-in for epfml/powersgd (``powersgd/__init__.py``): same public names.

    from powersgd_amd import PowerSGD, Config, optimizer_step

The compress/decompress hot path runs in libpsgd.so (hand-written HIP for gfx950,
C ABI in include/psgd.h); the factor all-reduce uses torch.distributed (RCCL on ROCm).
"""
import torch

from powersgd_amd.powersgd import Aggregator, AllReduce, Config, PowerSGD  # noqa: F401
from powersgd_amd.residual import Fp32ResidualPowerSGD  # noqa: F401
from powersgd_amd.utils import params_in_optimizer

__all__ = ["Aggregator", "AllReduce", "Config", "Fp32ResidualPowerSGD", "PowerSGD", "optimizer_step"]


def optimizer_step(optimizer: torch.optim.Optimizer, aggregator: Aggregator):
    """Aggregate gradients across workers with ``aggregator``, then take an optimizer
    step with the aggregate; afterwards ``p.grad`` holds the error-feedback buffer
    (reference powersgd/__init__.py:7-25). Global-norm clipping of the aggregate goes through the
    aggregator: ``PowerSGD(..., max_grad_norm=x)`` or its ``max_grad_norm`` attribute (the caller
    has no point between the aggregate and the step at which to clip). With
    ``PowerSGD(..., skip_nonfinite=True)`` a skipped (non-finite) step hands the optimizer zero
    gradients and leaves ``p.grad`` zero: plain SGD does not move, but the optimizer's own state
    (momentum, weight decay, step counts) still advances; ``aggregator.last_step_skipped`` is there
    for callers who want to act on it."""
    params = params_in_optimizer(optimizer)
    grads = [p.grad.data for p in params]  # type: ignore
    avg_grads = aggregator.aggregate(grads)  # subtracts the approximation from grads
    for p, g in zip(params, avg_grads):
        p.grad = g
    optimizer.step()
    for p, g in zip(params, grads):
        p.grad = g
