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

``fused=True`` runs the same step as ONE library call (psgd_aggregate_mixed, include/psgd.h)
wherever it applies (one process, a compressing step, rank bucket 1 / 2 / 4 / 16 / 32; rank bucket
8 and ranks above 32 run the three stages): the codec's final
pass stores the bf16 averages itself (no GATHER pass), and where a step is one gradient pass
(one iteration per step, odd steps) that pass also ingests the bf16 gradients (no ADD pass; on the
other steps the library launches the ADD). In a process group that runs over the library's own RCCL
communicator the one call is psgd_aggregate_mixed_comm: the output fold on every step, the ADD
always a launch of the library's, the uncompressed tensors all-reduced in fp32 and rounded in the
final launch. With ``PSGD_COMM=ipc`` it is psgd_aggregate_mixed_ipc over the codec's IPC exchange
session: the same output fold, and the last exchange stores the uncompressed tensors' averages as
bf16 itself. Bit for bit the three-stage flow above; every other case (``PSGD_COMM=torch``, gloo
without the IPC exchange, an ineligible plan) runs it.
"""
from __future__ import annotations

import ctypes
from abc import ABCMeta
from typing import List, Optional

import torch

from . import _lib
from .powersgd import (Aggregator, Config, PowerSGD, _check_max_grad_norm, _output_slab, _psgd_host,
                       _require_device, _stream, _views)
from .utils import is_distributed


class _ClipKeyword(ABCMeta):
    """``Fp32ResidualPowerSGD(params, config, fused=False, max_grad_norm=None, skip_nonfinite=False)``:
    the keywords are taken at the class call, ``max_grad_norm`` checked before any device work, and
    handed to the inner fp32 aggregator once it exists. ``__init__`` keeps the parameter list ``(params, config, fused)`` that existing callers
    and tests inspect."""

    def __call__(cls, *args, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, **kwargs):
        max_grad_norm = _check_max_grad_norm(max_grad_norm)
        obj = super().__call__(*args, **kwargs)
        obj.inner.max_grad_norm = max_grad_norm
        obj.inner.skip_nonfinite = skip_nonfinite  # (``PowerSGD.skip_nonfinite``, taken the same way)
        return obj


class Fp32ResidualPowerSGD(Aggregator, metaclass=_ClipKeyword):
    """``PowerSGD(params, config)`` for bfloat16 ``params`` on one GPU per process, with an fp32
    residual owned by the aggregator: ``residual`` (flat), ``views`` (per parameter), ``inner``
    (the fp32 ``PowerSGD`` over ``views``). ``fused``: take the one-call fused step where it
    applies (module docstring); same results, bit for bit. ``max_grad_norm`` (keyword, also a
    settable attribute): global-norm clipping by the inner aggregator (``PowerSGD.max_grad_norm``):
    the fp32 averages are clipped before the GATHER rounds them to bf16. ``skip_nonfinite`` (keyword):
    ``PowerSGD.skip_nonfinite`` of the inner aggregator: a skipped step zeroes the fp32 averages and
    ``residual`` before the GATHER, so the bf16 averages are zero too. While it is set every step runs
    the three stages, as under ``max_grad_norm``: the one-call forms have already rounded and stored
    by the time a verdict exists."""

    def __init__(self, params: List[torch.Tensor], config: Config, fused: bool = False):
        params = list(params)
        self.config = config
        self.fused = bool(fused)
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
        self._fused_state = None  # built by the first fused step

    @property
    def step_counter(self) -> int:
        return self.inner.step_counter

    @property
    def is_compressed_mask(self) -> List[bool]:
        return self.inner.is_compressed_mask

    @property
    def max_grad_norm(self) -> Optional[float]:
        """``PowerSGD.max_grad_norm`` of ``inner`` (settable). With a value the step runs the three
        stages even under ``fused=True``: the one-call forms store bf16 averages, and the clip
        belongs before that rounding."""
        return self.inner.max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value: Optional[float]) -> None:
        self.inner.max_grad_norm = value

    @property
    def skip_nonfinite(self) -> bool:
        """``PowerSGD.skip_nonfinite`` of ``inner`` (settable until the first ``aggregate``). While
        set, the step runs the three stages even under ``fused=True``."""
        return self.inner.skip_nonfinite

    @skip_nonfinite.setter
    def skip_nonfinite(self, on: bool) -> None:
        self.inner.skip_nonfinite = on

    @property
    def last_step_skipped(self):
        return self.inner.last_step_skipped

    @property
    def skipped_steps(self):
        return self.inner.skipped_steps

    @property
    def last_grad_norm(self):
        return self.inner.last_grad_norm

    @property
    def last_clip_coef(self):
        return self.inner.last_clip_coef

    def aggregate(self, gradients: List[torch.Tensor]) -> List[torch.Tensor]:
        """Average ``gradients`` (bf16) across workers; zeroes them (they are folded into the fp32
        residual, which keeps the compression error)."""
        if not isinstance(gradients, list):
            gradients = list(gradients)
        self._table.fill(gradients)  # count / dtype / device / shape / contiguity, as PowerSGD
        stream = _stream(self.device)
        if self.fused and self._fused_applies():
            return self._aggregate_fused(gradients, stream)
        self._add.add_list(self._table.comp_addr(), ctypes.addressof(self._res_ptrs), True, stream)
        avg = self.inner.aggregate(self.views)  # fp32; leaves the new residual in self.views
        _psgd_host.fill_list(avg, ctypes.addressof(self._out_ptrs), _lib.PSGD_F32, self._dev_index)
        outs = self._slab.get()
        self._gather.gather(self._slab.data_ptr(), ctypes.addressof(self._out_ptrs), stream)
        return outs

    def _fused_comm(self):
        """The library's own communicator when this process group runs over it (``PowerSGD.aggregate``'s
        choice: RCCL, not ``PSGD_COMM=ipc`` / ``torch``, not gloo), else None. Collective on first use."""
        codec = self.inner._powersgd
        if not is_distributed() or codec._ipc_mode():
            return None
        return codec._rccl_comm()

    def _fused_world(self):
        """The world size the communicator-route admission is asked for (psgd_plan_mixed_folds_comm):
        the process group's under ``PSGD_COMM=ipc`` (the exchange session spans it), the library
        communicator's over RCCL, None on every other transport."""
        if self.inner._powersgd._ipc_mode():
            return torch.distributed.get_world_size()
        comm = self._fused_comm()
        return None if comm is None else comm.world

    def _fused_applies(self) -> bool:
        """The step about to run compresses, on a plan the one-call form serves (both step parities:
        a plan is eligible or not as a whole): psgd_aggregate_mixed in one process,
        psgd_aggregate_mixed_comm in a process group that runs over the library's communicator,
        psgd_aggregate_mixed_ipc in one that runs over the IPC exchange."""
        inner = self.inner
        if inner.max_grad_norm is not None:  # clipped before the bf16 rounding: the three stages
            return False
        if inner.skip_nonfinite:  # the verdict comes after the step: zeroed before the GATHER
            return False
        if inner.step_counter + 1 <= self.config.start_compressing_after_num_steps:
            return False
        plan = inner._powersgd._plan
        if is_distributed():
            world = self._fused_world()
            if world is None:
                return False
            return plan.mixed_folds_comm(0, world)[1] == 1 and plan.mixed_folds_comm(1, world)[1] == 1
        return plan.mixed_folds(0)[1] == 1 and plan.mixed_folds(1)[1] == 1

    def fused_folds(self):
        """``(fold_in, fold_out)`` of the NEXT ``aggregate`` call: 1 where the ingest of the bf16
        gradients / the bf16 rounding of the averages will run inside the codec's own gradient
        pass (psgd_plan_mixed_folds; over a communicator or the IPC exchange
        psgd_plan_mixed_folds_comm: ``(0, 1)``);
        ``(0, 0)`` whenever that call runs the three-stage flow (``fused=False``, a warm-up step, a
        process group on another transport, a plan the fused call refuses, ``max_grad_norm`` or
        ``skip_nonfinite`` set)."""
        if not (self.fused and self._fused_applies()):
            return (0, 0)
        codec = self.inner._powersgd
        if is_distributed():
            return codec._plan.mixed_folds_comm(codec.step_counter, self._fused_world())
        return codec._plan.mixed_folds(codec.step_counter)

    def _aggregate_fused(self, gradients: List[torch.Tensor], stream: int) -> List[torch.Tensor]:
        """``PowerSGD.aggregate`` of ``inner`` on the residual, as psgd_aggregate_mixed[_flat]: the
        same bookkeeping (step counters, split by the compression mask, merge order), the bf16
        gradients consumed and the bf16 averages written inside the library call."""
        inner, codec = self.inner, self.inner._powersgd
        st = self._fused_state
        if st is None:
            mask = inner.is_compressed_mask
            shapes = [v.shape for v in self.views]
            st = self._fused_state = {
                # the bf16 gradients and the fp32 residual views, split like PowerSGD._split
                "grads": _psgd_host.PtrTable([list(s) for s in shapes], mask, _lib.PSGD_BF16, self._dev_index),
                "comp_slab": _output_slab([s for s, c in zip(shapes, mask) if c], _lib.PSGD_BF16, self._dev_index),
                "unc_slab": (_output_slab([s for s, c in zip(shapes, mask) if not c], _lib.PSGD_BF16, self._dev_index)
                             if inner._unc is not None else None),
            }
        st["grads"].fill(gradients)
        inner._table.fill(self.views)
        inner.step_counter += 1
        outs = st["comp_slab"].get()
        ipc = is_distributed() and codec._ipc_mode()
        if ipc:  # collective, once: exactly as PowerSGD.aggregate sets the exchange up
            codec._ipc_setup(inner._unc.numel if inner._unc is not None else 0)
        comm = self._fused_comm()
        kw = {}
        if inner._unc is not None:
            unc = st["unc_slab"].get()
            kw = dict(flat=inner._unc.plan, unc_bf16=st["grads"].unc_addr(), unc_residual=inner._table.unc_addr(),
                      flat_out=st["unc_slab"].data_ptr())
            outs = outs + unc
        if ipc:
            codec._plan.aggregate_mixed_ipc(st["grads"].comp_addr(), inner._table.comp_addr(),
                                            st["comp_slab"].data_ptr(), codec.step_counter, stream, **kw)
        elif comm is not None:
            codec._plan.aggregate_mixed_comm(st["grads"].comp_addr(), inner._table.comp_addr(),
                                             st["comp_slab"].data_ptr(), codec.step_counter, comm, stream, **kw)
        else:
            codec._plan.aggregate_mixed(st["grads"].comp_addr(), inner._table.comp_addr(), st["comp_slab"].data_ptr(),
                                        codec.step_counter, stream, **kw)
        codec.step_counter += 1
        return [outs[i] for i in inner._order]

    def close(self) -> None:
        """Collective: release the codec's multi-GPU transports (PowerSGD.close)."""
        self.inner.close()
