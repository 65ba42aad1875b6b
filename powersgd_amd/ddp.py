"""DistributedDataParallel communication hook running this package's PowerSGD codec.

The reference drives PowerSGD from the optimizer (``optimizer_step``, powersgd/__init__.py:
7-25): ONE ``PowerSGD`` over all parameters in optimizer order, the error-feedback residual
kept in ``p.grad`` so the next backward adds onto it (README.md:39-42). Under
``DistributedDataParallel`` the gradients reach the aggregator bucket by bucket through
``register_comm_hook`` (the paper code plugs PowerSGD in that way, paper-code/
train_pytorch.py:106-131). This adapter reproduces the reference flow exactly, independent of
how DDP buckets the parameters (and of its bucket rebuild after the first iteration):

* the state owns one ``PowerSGD`` over ``params`` in the given (optimizer) order — the same
  compression mask, shape-group batching, P/Q state and step counter as the reference's
  ``PowerSGD(params, config)`` (reference :41-105, :113-275);
* it owns the error-feedback residual per parameter (one flat buffer): each bucket's fresh
  gradients are ADDED to their parameters' residual (what autograd's accumulation into
  ``p.grad`` does in the reference flow);
* a bucket's future completes when the LAST bucket of the iteration has arrived: then one
  ``aggregate`` runs over all parameters (its factor all-reduces on the default process group,
  reference :207) and every pending bucket receives its averaged approximation in its own
  layout. DDP waits on all bucket futures only after backward has launched every hook, so the
  deferral is legal; it trades DDP's per-bucket overlap for the reference's exact semantics.

Bucket plumbing is native (include/psgd.h ``psgd_runs_*``): per DDP bucket layout a run table
(bucket offset, parameter, length: one run per parameter, 64-bit offsets) drives one HIP launch
that adds the bucket into the residual and, at completion, one that gathers the averages back
into the bucket buffer. No index maps, no full-size copy, no limit on the element count.

Because the residual lives in the state (not in ``p.grad``), the training loop zeroes
gradients as usual:

    state = PowerSGDState(Config(rank=2, num_iters_per_step=2, start_compressing_after_num_steps=0),
                          params=[p for p in model.parameters()])
    ddp_model.register_comm_hook(state, powersgd_hook)
    loss.backward(); optimizer.step(); optimizer.zero_grad()
"""
import ctypes
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import _lib
from .powersgd import Config, PowerSGD, _DTYPES, _check_max_grad_norm, _psgd_host, _require_device, _stream
from .utils import is_distributed


class _BucketRuns:
    """The run table of one DDP bucket layout (one run per parameter: bucket offset, parameter
    index, length), bound to device memory (psgd_runs_*)."""

    def __init__(self, key, buf: torch.Tensor, grads, idx, ntensors: int, code: int, dev_index: int,
                 bucket_code: Optional[int] = None):
        self.key = key
        esz = buf.element_size()
        self.offs = [(g.data_ptr() - buf.data_ptr()) // esz for g in grads]
        self.idx = list(idx)
        self.lens = [g.numel() for g in grads]
        # bucket_code: the bucket's dtype where it differs from the residual's (bf16 over fp32)
        self.runs = _lib.Runs(self.offs, self.idx, [0] * len(idx), self.lens, ntensors, code, bucket_code)
        self.ws = torch.empty(self.runs.workspace_bytes(), dtype=torch.uint8, device=buf.device)
        self.runs.bind(dev_index, self.ws.data_ptr())


class _ClipKeyword(type):
    """``PowerSGDState(config, params, ..., fused=False, max_grad_norm=None, skip_nonfinite=False)``: the
    keywords are taken at the class call, ``max_grad_norm`` checked before any device work, and
    handed to the inner aggregator once it exists (as ``Fp32ResidualPowerSGD`` takes them). ``__init__`` keeps the parameter list ``(config,
    params, process_group, residual_dtype, fused)`` that existing callers and tests inspect."""

    def __call__(cls, *args, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, **kwargs):
        max_grad_norm = _check_max_grad_norm(max_grad_norm)
        obj = super().__call__(*args, **kwargs)
        obj.powersgd.max_grad_norm = max_grad_norm
        obj.powersgd.skip_nonfinite = skip_nonfinite  # (``PowerSGD.skip_nonfinite``, taken the same way)
        return obj


class PowerSGDState(metaclass=_ClipKeyword):
    """Hook state: one codec + residual buffer over ``params`` (the optimizer's order).

    ``residual_dtype=torch.float32`` with bfloat16 parameters keeps the error-feedback residual in
    fp32: each bf16 bucket is upcast exactly and added in fp32 (a bf16 residual drops every fresh
    component below 2^-8 of the element it lands on), the codec and the uncompressed average run
    in fp32 on the residual, and DDP gets the bf16 rounding of the fp32 average back. ``None``
    (default): the residual has the parameters' dtype. 4 bytes of state per parameter instead
    of 2.

    ``fused=True`` (bfloat16 parameters with ``residual_dtype=torch.float32`` only) completes an
    iteration in ONE library call wherever it applies (psgd_aggregate_mixed_comm_dst, or
    psgd_aggregate_mixed_ipc_dst under ``PSGD_COMM=ipc``; include/psgd.h): the codec's final pass
    stores the bf16 rounding of each parameter's average straight into that parameter's view of its
    DDP bucket, so no fp32 output slab is written and no per-bucket gather runs. Bit for bit the
    three stages it replaces. It applies on a compressing step, in a process group that runs over
    the library's own communicator or over the IPC exchange (not ``PSGD_COMM=torch``, not gloo
    without the IPC exchange), on a plan the call serves (rank bucket 1 / 2 / 4 / 16 / 32; not 8, not ranks above 32); every other
    completion runs the three stages (``fused_folds()`` tells which).

    ``state.direct_store = True`` (float32 parameters with a float32 residual, ``fused=False``; set
    before the first backward) is the same one-call completion for the default fp32 hook
    (psgd_aggregate_comm_dst, or psgd_aggregate_ipc_dst under ``PSGD_COMM=ipc``): the final pass
    stores each parameter's fp32 average straight into its view of its DDP bucket, at rank buckets
    1 to 32. Bit for bit the three stages; ``direct_store_applies()`` tells whether the next
    completion takes it (a compressing step, the library's communicator or the IPC exchange, a plan
    ``Plan.dst_ok`` reports 1 for). Opt-in: the default is ``False``.

    ``max_grad_norm`` (keyword only; also a settable attribute, as on ``PowerSGD``: positive, ``inf``
    to measure only, or ``None``): what the hook hands back to DDP in the buckets, over all
    parameters of the iteration, is clipped by its global L2 norm inside the library, on the codec's
    stream with no host synchronisation: what ``torch.nn.utils.clip_grad_norm_(params, x)`` would do
    after ``backward()``, ``coef = min(1, x / (norm + 1e-6))``. The caller must NOT clip again. A
    non-finite norm gives ``coef = NaN`` and leaves everything untouched; the residual is never
    touched. ``last_grad_norm`` / ``last_clip_coef``: 0-dim float64 device tensors, views of one
    two-double result buffer that the next completion overwrites; ``None`` until the first clipped
    completion. What each completion form does with it:

    * three stages: the inner ``PowerSGD`` clips the averages (compressed slab and uncompressed
      slab; warm-up steps through the same call) before they are gathered into the buckets; with
      bf16 parameters over an fp32 residual the fp32 averages are clipped before the gather's bf16
      rounding (``Fp32ResidualPowerSGD``'s rule);
    * ``fused=True``: every completion runs the three stages while ``max_grad_norm`` is set (the
      one-call form has rounded to bf16 by the time a norm exists); ``fused_folds()`` reports
      ``(0, 0)``;
    * ``direct_store``: the one-call completion is followed by psgd_clip_dst on the same stream: the
      norm from the low-rank factors and the staged uncompressed sums, the averages scaled where
      they lie in the buckets, and only when the norm exceeds the threshold. Bit for bit the three
      stages with the clip. It also needs ``Plan.clip_dst_ok()``; otherwise the completion runs
      the three stages with the clip.

    ``skip_nonfinite`` (keyword only; ``PowerSGD.skip_nonfinite`` of the inner aggregator, settable
    until the first backward): an iteration whose aggregates are not finite is skipped on the
    device, with no host synchronisation: the buckets come back all zero, ``residual`` is zeroed and
    P / Q go back to their seed; ``last_step_skipped`` / ``skipped_steps`` are the inner
    aggregator's. While it is set every completion runs the three stages (the inner aggregator
    zeroes the averages and the residual views before they are gathered into the buckets):
    ``fused_folds()`` reports ``(0, 0)`` and ``direct_store_applies()`` ``False``, since the one-call
    forms have already stored into the buckets by the time a verdict exists."""

    fused = False  # (class default: the three-stage completion)
    _direct = False

    def __init__(self, config: Config, params, process_group=None, residual_dtype=None, fused=False):
        if process_group is not None and process_group is not dist.group.WORLD:
            raise ValueError("powersgd_hook all-reduces on the default process group (reference :207)")
        self.config = config
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        if not self.params:
            raise IndexError("list index out of range")  # the reference's PowerSGD on []
        self._index: Dict[int, int] = {id(p): i for i, p in enumerate(self.params)}
        numel = sum(p.numel() for p in self.params)
        p0 = self.params[0]
        # the run-table kernels (psgd_runs_*) read buckets and write the residual at ONE element
        # size, the state's: a mixed-dtype parameter list would index them at the wrong width
        mixed = [i for i, p in enumerate(self.params) if p.dtype != p0.dtype]
        if mixed:
            raise RuntimeError(f"powersgd_hook needs one gradient dtype: parameter {mixed[0]} is "
                               f"{self.params[mixed[0]].dtype}, parameter 0 is {p0.dtype}")
        if residual_dtype is not None and not (residual_dtype == torch.float32
                                               and p0.dtype in (torch.float32, torch.bfloat16)):
            raise ValueError(f"residual_dtype must be None, or torch.float32 with float32 / bfloat16 parameters; "
                             f"got {residual_dtype} with {p0.dtype} parameters")
        self.fused = bool(fused)
        if self.fused and not (p0.dtype == torch.bfloat16 and residual_dtype == torch.float32):
            raise ValueError(f"fused=True needs bfloat16 parameters with residual_dtype=torch.float32; got "
                             f"{p0.dtype} parameters with residual_dtype={residual_dtype}")
        self._dev_index = _require_device(p0.device)
        if p0.dtype not in _DTYPES:
            raise RuntimeError(f"powersgd_hook supports float32, bfloat16 and float64 gradients, got {p0.dtype}")
        res_dtype = p0.dtype if residual_dtype is None else residual_dtype
        # the residual's dtype code (run tables' tensor side, the codec, the averages) and, where the
        # DDP buckets' dtype differs from it (bf16 buckets over an fp32 residual), the buckets'
        self._code = _DTYPES[res_dtype]
        self._bucket_code = _DTYPES[p0.dtype] if p0.dtype != res_dtype else None
        self.residual = torch.zeros(numel, dtype=res_dtype, device=p0.device)
        self.views: List[torch.Tensor] = []
        off = 0
        for p in self.params:
            self.views.append(self.residual[off:off + p.numel()].view(p.shape))
            off += p.numel()
        # per-parameter pointer tables (host arrays handed to psgd_runs_*): the residual views
        # (fixed) and the latest averaged outputs (refilled natively at every completion)
        self._res_ptrs = _lib.ptr_array([v.data_ptr() for v in self.views])
        self._out_ptrs = _lib.ptr_array([0] * len(self.views))
        # per DDP bucket index: the run table of its LATEST layout only (DDP rebuilds its buckets
        # after the first iteration; the old tables are dropped)
        self._runs: Dict[int, _BucketRuns] = {}
        self.powersgd = PowerSGD(self.views, config)
        # norm and coefficient of the latest clipped completion (two doubles; made by the first one
        # and shared with the inner aggregator, so every completion form writes the same buffer)
        self._clip_result: Optional[torch.Tensor] = None
        self._seen = [False] * len(self.params)
        self._nseen = 0
        self._pending: List[tuple] = []
        # fused / direct_store: per parameter its gradient view inside the pending bucket (the
        # destination of its average), and their native split by the compression mask (built by the
        # first one-call completion)
        self._dst: List[Optional[torch.Tensor]] = [None] * len(self.params)
        self._dst_table = None

    def _arrive(self, bucket: "dist.GradBucket") -> "torch.futures.Future[torch.Tensor]":
        fut: torch.futures.Future = torch.futures.Future()
        try:
            params, grads = bucket.parameters(), bucket.gradients()
            idx = []
            for p, g in zip(params, grads):
                i = self._index.get(id(p))
                if i is None:
                    raise RuntimeError("DDP bucket holds a parameter that PowerSGDState was not given")
                if self._seen[i]:
                    raise RuntimeError("parameter reached powersgd_hook twice in one iteration")
                idx.append(i)
            buf = bucket.buffer()
            if buf.dtype != self.params[0].dtype:
                # DDP buckets carry the gradients' dtype (the parameters'; the residual's may be
                # fp32 over bf16 gradients); anything else (e.g. a bf16 bucket under an fp32
                # state) would be read and written at the wrong element size
                raise RuntimeError(f"powersgd_hook: DDP bucket dtype {buf.dtype} differs from the state's "
                                   f"gradient dtype {self.params[0].dtype}")
            runs = self._bucket_runs(bucket.index(), buf, grads, idx)
            self._ef_add(buf, runs)
            for i in idx:
                self._seen[i] = True
                self._nseen += 1
            if self.fused or self._direct:
                for i, g in zip(idx, grads):
                    self._dst[i] = g.view(self.params[i].shape)
            self._pending.append((buf, runs, fut))
            if self._nseen == len(self.params):
                self._complete()
            elif bucket.is_last():
                # DDP's last bucket arrived but some trainable parameter never did (e.g. one
                # DDP ignores): no aggregate can run, and waiting would hang DDP's backward
                missing = [i for i, s in enumerate(self._seen) if not s]
                raise RuntimeError(f"powersgd_hook: {len(missing)} parameter(s) given to PowerSGDState never "
                                   f"reached a DDP bucket (first index {missing[0]}); give the state exactly "
                                   "the parameters DDP reduces")
        except Exception as e:
            self._fail(e, fut)
            raise
        return fut

    @property
    def max_grad_norm(self) -> Optional[float]:
        return self.powersgd.max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value: Optional[float]) -> None:
        self.powersgd.max_grad_norm = value

    @property
    def skip_nonfinite(self) -> bool:
        return self.powersgd.skip_nonfinite

    @skip_nonfinite.setter
    def skip_nonfinite(self, on: bool) -> None:
        if bool(on) != self.powersgd.skip_nonfinite and self._pending:
            raise ValueError("skip_nonfinite is set before the first backward")
        self.powersgd.skip_nonfinite = on

    @property
    def last_step_skipped(self) -> Optional[torch.Tensor]:
        return self.powersgd.last_step_skipped

    @property
    def skipped_steps(self) -> Optional[torch.Tensor]:
        return self.powersgd.skipped_steps

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        return self.powersgd.last_grad_norm

    @property
    def last_clip_coef(self) -> Optional[torch.Tensor]:
        return self.powersgd.last_clip_coef

    def _clip_buffer(self) -> torch.Tensor:
        """The state's result buffer, handed to the inner aggregator as its own."""
        if self._clip_result is None:
            inner = self.powersgd
            self._clip_result = torch.zeros(2, dtype=torch.float64, device=self.residual.device)
            inner._clip_result = self._clip_result
            inner.last_grad_norm, inner.last_clip_coef = self._clip_result[0], self._clip_result[1]
        return self._clip_result

    @property
    def direct_store(self) -> bool:
        return self._direct

    @direct_store.setter
    def direct_store(self, on: bool) -> None:
        on = bool(on)
        if on and not (self.params[0].dtype == torch.float32 and self.residual.dtype == torch.float32
                       and not self.fused):
            raise ValueError(f"direct_store needs float32 parameters with a float32 residual and fused=False; got "
                             f"{self.params[0].dtype} parameters, a {self.residual.dtype} residual, fused={self.fused}")
        if on != self._direct and (self._pending or self.powersgd.step_counter > 0):
            raise ValueError("direct_store is set before the first backward")
        self._direct = on

    def _fail(self, err: Exception, fut: "torch.futures.Future") -> None:
        """Fail this iteration: every pending bucket future (and this one) gets the exception, so
        DDP's wait raises instead of hanging, and the next iteration starts clean."""
        pending, self._pending = self._pending, []
        self._seen = [False] * len(self.params)
        self._nseen = 0
        self._dst = [None] * len(self.params)
        for *_, f in pending:
            if not f.done():
                f.set_exception(err)
        if not fut.done():
            fut.set_exception(err)

    def _bucket_runs(self, bucket_index: int, buf: torch.Tensor, grads, idx) -> _BucketRuns:
        """The bucket's run table (one run per parameter: bucket offset -> parameter, length),
        built once per bucket layout; only the bucket's latest layout is kept."""
        key = (buf.numel(), tuple(idx), tuple((g.data_ptr() - buf.data_ptr()) // buf.element_size() for g in grads))
        hit = self._runs.get(bucket_index)
        if hit is not None and hit.key == key:
            return hit
        self._runs.pop(bucket_index, None)
        r = self._new_runs(key, buf, grads, idx)
        self._runs[bucket_index] = r
        return r

    def _new_runs(self, key, buf, grads, idx) -> _BucketRuns:
        return _BucketRuns(key, buf, grads, idx, len(self.params), self._code, self._dev_index, self._bucket_code)

    def _ef_add(self, buf: torch.Tensor, runs: _BucketRuns) -> None:
        """Error feedback: residual += the bucket's fresh gradients, the whole bucket in one launch
        (autograd's accumulation into p.grad in the reference flow, README.md:39-42)."""
        runs.runs.add(buf.data_ptr(), ctypes.addressof(self._res_ptrs), _stream(buf.device))

    def _gather(self, pending, outs) -> None:
        """The averages, parameter by parameter, straight into each pending bucket's buffer (its
        own layout), one launch per bucket on the codec's stream."""
        _psgd_host.fill_list(outs, ctypes.addressof(self._out_ptrs), self._code, self._dev_index)
        stream = _stream(self.residual.device)
        for buf, runs, _ in pending:
            runs.runs.gather(buf.data_ptr(), ctypes.addressof(self._out_ptrs), stream)

    def _fused_comm(self):
        """The library's own communicator when this process group runs over it (``PowerSGD.aggregate``'s
        choice: RCCL, not ``PSGD_COMM=ipc`` / ``torch``, not gloo), else None. Collective on first use."""
        codec = self.powersgd._powersgd
        if not is_distributed() or codec._ipc_mode():
            return None
        return codec._rccl_comm()

    def _fused_ipc(self) -> bool:
        """This process group runs over the codec's IPC exchange (``PSGD_COMM=ipc``)."""
        return is_distributed() and self.powersgd._powersgd._ipc_mode()

    def _fused_applies(self) -> bool:
        """The completion about to run compresses, over the library's communicator or the IPC
        exchange, on a plan psgd_aggregate_mixed_comm_dst / psgd_aggregate_mixed_ipc_dst serves (both
        step parities: a plan is eligible as a whole). Never while ``max_grad_norm`` is set: the
        averages are clipped in fp32, before the bf16 rounding; never while ``skip_nonfinite`` is set."""
        inner = self.powersgd
        if inner.max_grad_norm is not None or inner.skip_nonfinite:
            return False
        if inner.step_counter + 1 <= self.config.start_compressing_after_num_steps:
            return False
        if self._fused_ipc():
            world = dist.get_world_size()
        else:
            comm = self._fused_comm()
            if comm is None:
                return False
            world = comm.world
        plan = inner._powersgd._plan
        return plan.mixed_folds_dst(0, world) == 1 and plan.mixed_folds_dst(1, world) == 1

    def fused_folds(self):
        """``(fold_in, fold_out)`` of the NEXT completion: ``(0, 1)`` when it takes the one-call form
        (the bf16 rounding of the averages runs inside the codec's final pass; the per-bucket ADD is
        never folded: it runs at bucket arrival, under backward), ``(0, 0)`` when it runs the three
        stages (``fused=False``, a warm-up step, another transport, a plan the call refuses,
        ``max_grad_norm`` or ``skip_nonfinite`` set)."""
        return (0, 1) if self.fused and self._fused_applies() else (0, 0)

    def _complete_fused(self) -> None:
        """``PowerSGD.aggregate`` of the codec on the residual views as one library call: the same
        bookkeeping (both step counters, the split by the compression mask), the bf16 averages
        stored by the final pass into the pending buckets' gradient views. No ``_gather``."""
        inner, codec = self.powersgd, self.powersgd._powersgd
        if self._dst_table is None:
            self._dst_table = _psgd_host.PtrTable([list(v.shape) for v in self.views], inner.is_compressed_mask,
                                                  _lib.PSGD_BF16, self._dev_index)
        self._dst_table.fill(self._dst)
        inner.step_counter += 1
        inner._table.fill(self.views)
        kw = {}
        if inner._unc is not None:
            kw = dict(flat=inner._unc.plan, unc_residual=inner._table.unc_addr(),
                      unc_dst_bf16=self._dst_table.unc_addr())
        if self._fused_ipc():
            # collective, once: exactly as PowerSGD.aggregate sets the exchange up
            codec._ipc_setup(inner._unc.numel if inner._unc is not None else 0)
            codec._plan.aggregate_mixed_ipc_dst(inner._table.comp_addr(), self._dst_table.comp_addr(),
                                                codec.step_counter, _stream(self.residual.device), **kw)
        else:
            codec._plan.aggregate_mixed_comm_dst(inner._table.comp_addr(), self._dst_table.comp_addr(),
                                                 codec.step_counter, self._fused_comm(), _stream(self.residual.device),
                                                 **kw)
        codec.step_counter += 1
        pending, self._pending = self._pending, []
        self._seen = [False] * len(self.params)
        self._nseen = 0
        self._dst = [None] * len(self.params)
        for buf, _, fut in pending:
            fut.set_result(buf)

    def direct_store_applies(self) -> bool:
        """The NEXT completion takes the one-call form of ``direct_store``: it is set, the step
        compresses, the process group runs over the library's communicator or the IPC exchange, and
        the plan is one psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst serve (with ``max_grad_norm``
        set: and psgd_clip_dst, ``Plan.clip_dst_ok``). Never while ``skip_nonfinite`` is set."""
        if not self._direct:
            return False
        inner = self.powersgd
        if inner.skip_nonfinite:  # the verdict comes after the step: the three stages
            return False
        if inner.step_counter + 1 <= self.config.start_compressing_after_num_steps:
            return False
        if self._fused_ipc():
            world = dist.get_world_size()
        else:
            comm = self._fused_comm()
            if comm is None:
                return False
            world = comm.world
        plan = inner._powersgd._plan
        if inner.max_grad_norm is not None and plan.clip_dst_ok() != 1:
            return False
        return plan.dst_ok(0, world) == 1 and plan.dst_ok(1, world) == 1

    def _complete_direct(self) -> None:
        """``PowerSGD.aggregate`` of the codec on the residual views as one library call, as
        ``_complete_fused``: the same bookkeeping, the fp32 averages stored by the final pass into the
        pending buckets' gradient views. No ``_gather``, no output slab. With ``max_grad_norm``
        set, psgd_clip_dst follows on the same stream, on the destination tables just filled."""
        inner, codec = self.powersgd, self.powersgd._powersgd
        stream = _stream(self.residual.device)
        if self._dst_table is None:
            self._dst_table = _psgd_host.PtrTable([list(v.shape) for v in self.views], inner.is_compressed_mask,
                                                  _lib.PSGD_F32, self._dev_index)
        self._dst_table.fill(self._dst)
        inner.step_counter += 1
        inner._table.fill(self.views)
        kw = {}
        if inner._unc is not None:
            kw = dict(flat=inner._unc.plan, unc=inner._table.unc_addr(), unc_dst=self._dst_table.unc_addr())
        if self._fused_ipc():
            # collective, once: exactly as PowerSGD.aggregate sets the exchange up
            codec._ipc_setup(inner._unc.numel if inner._unc is not None else 0)
            codec._plan.aggregate_ipc_dst(inner._table.comp_addr(), self._dst_table.comp_addr(), codec.step_counter,
                                          stream, **kw)
            world = dist.get_world_size()
        else:
            comm = self._fused_comm()
            codec._plan.aggregate_comm_dst(inner._table.comp_addr(), self._dst_table.comp_addr(), codec.step_counter,
                                           comm, stream, **kw)
            world = comm.world
        if inner.max_grad_norm is not None:
            ckw = dict(flat=kw["flat"], unc_dst=kw["unc_dst"]) if kw else {}
            codec._plan.clip_dst(codec.step_counter, world, self._dst_table.comp_addr(), inner.max_grad_norm,
                                 self._clip_buffer().data_ptr(), stream, **ckw)
        codec.step_counter += 1
        pending, self._pending = self._pending, []
        self._seen = [False] * len(self.params)
        self._nseen = 0
        self._dst = [None] * len(self.params)
        for buf, _, fut in pending:
            fut.set_result(buf)

    def _complete(self) -> None:
        if self.fused:
            if self._fused_applies():
                return self._complete_fused()
            self._dst = [None] * len(self.params)
        if self._direct:
            if self.direct_store_applies():
                return self._complete_direct()
            self._dst = [None] * len(self.params)
        if getattr(self.powersgd, "max_grad_norm", None) is not None:
            self._clip_buffer()
        outs = self.powersgd.aggregate(self.views)  # leaves the new residual in self.views (clipped: outs)
        pending, self._pending = self._pending, []
        self._seen = [False] * len(self.params)
        self._nseen = 0
        # the gathers read `outs` on the stream; the codec reuses its output buffer only at a later
        # aggregate (same stream) once no view of it is referenced: queued before that, safe
        self._gather(pending, outs)
        for buf, _, fut in pending:
            fut.set_result(buf)


def powersgd_hook(state: PowerSGDState, bucket: dist.GradBucket) -> torch.futures.Future[torch.Tensor]:
    """``DistributedDataParallel.register_comm_hook`` hook: the reference's PowerSGD flow."""
    return state._arrive(bucket)
