"""``Fp32ResidualPowerSGD``: PowerSGD for bfloat16 gradients with the error-feedback residual
kept in fp32 (the ``optimizer_step`` flow; the DDP hook's counterpart is
``PowerSGDState(residual_dtype=torch.float32)``).

``PowerSGD`` on bf16 gradients keeps the residual where the reference keeps it, in ``p.grad``:
the final pass rounds it to bf16 and autograd's next accumulation is a bf16 add, which drops
every fresh component below 2^-8 of the residual element it lands on, every step. Here the
aggregator owns the residual (one flat fp32 buffer, the parameters back to back) and the
gradients are *consumed*:

    residual += float(gradients); gradients = 0     one native pass (psgd_runs_add_list)
    averages  = PowerSGD(views).aggregate(views)    the fp32 codec, residual left in ``views``
    return bf16(averages)                           one native pass (psgd_runs_gather)

so ``optimizer_step`` works unchanged: it restores ``p.grad`` to the (zeroed) gradients and the
next backward accumulates fresh gradients only. Cost against ``PowerSGD`` on the same bf16
gradients: the two element-wise passes, an fp32 codec step, 4 bytes of state per parameter.
"""
from __future__ import annotations

import ctypes
from typing import List

import torch

from . import _lib
from .powersgd import Aggregator, Config, PowerSGD, _output_slab, _psgd_host, _require_device, _stream, _views


class Fp32ResidualPowerSGD(Aggregator):
    """``PowerSGD(params, config)`` for bfloat16 ``params`` on one GPU per process, with an fp32
    residual owned by the aggregator: ``residual`` (flat), ``views`` (per parameter), ``inner``
    (the fp32 ``PowerSGD`` over ``views``)."""

    def __init__(self, params: List[torch.Tensor], config: Config):
        params = list(params)
        self.config = config
        self.device = params[0].device  # IndexError on an empty list, as PowerSGD
        bad = [p.dtype for p in params if p.dtype != torch.bfloat16]
        if bad:
            raise RuntimeError(f"Fp32ResidualPowerSGD is for bfloat16 gradients, got {bad[0]}: use PowerSGD, whose "
                               "residual already has the gradients' precision")
        self._dev_index = _require_device(self.device)
        shapes = [p.shape for p in params]
        numels = [s.numel() for s in shapes]
        n = len(shapes)
        self.residual = torch.zeros(sum(numels), dtype=torch.float32, device=self.device)
        self.views = _views(self.residual, shapes)
        self.inner = PowerSGD(self.views, config)
        # checks + source pointers of the bf16 gradients in one native pass (as PowerSGD's)
        self._table = _psgd_host.PtrTable([list(s) for s in shapes], [True] * n, _lib.PSGD_BF16, self._dev_index)
        self._res_ptrs = _lib.ptr_array([v.data_ptr() for v in self.views])
        self._out_ptrs = _lib.ptr_array([0] * n)
        # ADD: one run per parameter, gradient i -> view i (source-table form, sources zeroed)
        self._add = _lib.Runs([0] * n, list(range(n)), [0] * n, numels, n, _lib.PSGD_F32, _lib.PSGD_BF16,
                              source=list(range(n)), nsources=n)
        # GATHER: fp32 output i -> its range of the flat bf16 output buffer (dense, tensor order)
        offs = [sum(numels[:i]) for i in range(n)]
        self._gather = _lib.Runs(offs, list(range(n)), [0] * n, numels, n, _lib.PSGD_F32, _lib.PSGD_BF16)
        self._ws = []
        for r in (self._add, self._gather):
            ws = torch.empty(r.workspace_bytes(), dtype=torch.uint8, device=self.device)
            r.bind(self._dev_index, ws.data_ptr())
            self._ws.append(ws)
        self._slab = _output_slab(shapes, _lib.PSGD_BF16, self._dev_index)

    @property
    def step_counter(self) -> int:
        return self.inner.step_counter

    @property
    def is_compressed_mask(self) -> List[bool]:
        return self.inner.is_compressed_mask

    def aggregate(self, gradients: List[torch.Tensor]) -> List[torch.Tensor]:
        """Average ``gradients`` (bf16) across workers; zeroes them (they are folded into the fp32
        residual, which keeps the compression error)."""
        if not isinstance(gradients, list):
            gradients = list(gradients)
        self._table.fill(gradients)  # count / dtype / device / shape / contiguity, as PowerSGD
        stream = _stream(self.device)
        self._add.add_list(self._table.comp_addr(), ctypes.addressof(self._res_ptrs), True, stream)
        avg = self.inner.aggregate(self.views)  # fp32; leaves the new residual in self.views
        _psgd_host.fill_list(avg, ctypes.addressof(self._out_ptrs), _lib.PSGD_F32, self._dev_index)
        outs = self._slab.get()
        self._gather.gather(self._slab.data_ptr(), ctypes.addressof(self._out_ptrs), stream)
        return outs

    def close(self) -> None:
        """Collective: release the codec's multi-GPU transports (PowerSGD.close)."""
        self.inner.close()
