"""What one training step's communication + optimizer half costs, the alternatives interleaved in one process.

    python tools/sgd_step_time.py [--steps 50] [--warmup 10] [--rounds 7] [--out profiles/sgd_step/sgd_step_time.jsonl]

One GPU, a one-rank process group over the library's communicator (the transport ``sgd_step`` serves).
Shapes: cfg2 (rank 1), cfg3 (rank 4) and cfg3's at rank 16, all with two iterations per step.
Cases (each its own parameters, optimizer and aggregator over the same shapes and gradient sets;
``torch.optim.SGD(lr=0.1, momentum=0.9, weight_decay=5e-4)``):
  a  optimizer_step, torch's default SGD (foreach)
  b  optimizer_step, SGD(fused=True)                     (where this torch offers it)
  c  sgd_step in its one-call form                        (psgd_aggregate_comm_sgd)
  d  aggregate, then psgd_sgd_update on the averages      (the sequence c is defined through, from Python)
Every step first points p.grad at the next gradient set (the same host work in every case). Every
round times `steps` steps of each case between two device events, in the order a..d; cold: four
gradient sets rotated (more than the Infinity Cache holds), warm: one. The report is the per-step
median, min and max over the rounds; a difference counts only beyond the spread (max - min) of both
cases. One JSON line per (shapes, cache). ``--ulp``: also the largest ulp distance between sgd_step and
optimizer_step + torch's SGD on the cfg3 shapes, two steps from identical state (measured, not asserted)."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from powersgd_amd import Config, PowerSGD, _lib, optimizer_step, sgd_step, sgd_step_applies  # noqa: E402
from powersgd_amd.powersgd import _stream  # noqa: E402
from powersgd_amd.workloads import CONFIGS, hash_tensors  # noqa: E402

HP = dict(lr=0.1, momentum=0.9, weight_decay=5e-4)
SHAPES = [("cfg2_resnet50_r1", 1), ("cfg3_resnet50_r4", 4), ("cfg3_resnet50_r4", 16)]


class Case:
    def __init__(self, shapes, rank, mcr, dev, seed=5, **opt_kw):
        gen = torch.Generator().manual_seed(seed)
        self.params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
        self.opt = torch.optim.SGD(self.params, **HP, **opt_kw)
        self.agg = PowerSGD(self.params, Config(rank, mcr, 2, 0))

    def point(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = g


class Sequence(Case):
    """aggregate + psgd_sgd_update: tables built once (the averages live in the codec's slabs)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bufs = [torch.zeros_like(p) for p in self.params]
        self.numel = [p.numel() for p in self.params]
        self.p = _lib.ptr_array([p.data_ptr() for p in self.params])
        self.b = _lib.ptr_array([b.data_ptr() for b in self.bufs])
        self.first = True

    def step(self, grads):
        outs = self.agg.aggregate(grads)
        g = _lib.ptr_array([o.data_ptr() for o in outs])
        hyper = _lib.sgd_hyper([(HP["lr"], HP["momentum"], 0.0, HP["weight_decay"], False, self.first)] * len(outs))
        self.first = False
        _lib.sgd_update(self.agg._powersgd._plan, ctypes.addressof(g), ctypes.addressof(self.p), ctypes.addressof(self.b),
                        self.numel, hyper, _stream(self.agg.device))


def monotone(x):
    """fp32 bits as integers ordered like the values (ulp distance = difference)."""
    i = x.contiguous().view(torch.int32).long()
    return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))


def ulp_distance(dev):
    c = CONFIGS["cfg3_resnet50_r4"]
    a, b = Case(c["shapes"], 4, c["mcr"], dev), Case(c["shapes"], 4, c["mcr"], dev)
    worst = {"p": 0, "buf": 0}
    for t in range(2):  # step 0: the buffers' first step
        for x, y in zip(a.params, b.params):  # identical state before every step
            x.data.copy_(y.data)
            if "momentum_buffer" in b.opt.state[y]:
                a.opt.state[x]["momentum_buffer"].copy_(b.opt.state[y]["momentum_buffer"])
        for case in (a, b):
            case.point([torch.from_numpy(x).to(dev) for x in hash_tensors(c["shapes"], seed=40 + t)])
        assert sgd_step_applies(a.opt, a.agg)
        sgd_step(a.opt, a.agg)
        optimizer_step(b.opt, b.agg)
        torch.cuda.synchronize()
        for x, y in zip(a.params, b.params):
            worst["p"] = max(worst["p"], int((monotone(x.data) - monotone(y.data)).abs().max()))
            bx, by = a.opt.state[x]["momentum_buffer"], b.opt.state[y]["momentum_buffer"]
            worst["buf"] = max(worst["buf"], int((monotone(bx) - monotone(by)).abs().max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ulp", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    store = os.path.join(tempfile.mkdtemp(), "init")
    torch.distributed.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1, device_id=dev)
    lines = []
    try:
        for name, rank in SHAPES:
            c = CONFIGS[name]
            for cache, nsets in (("cold", 4), ("warm", 1)):
                sets = [[torch.from_numpy(x).to(dev) for x in hash_tensors(c["shapes"], seed=11 + k)] for k in range(nsets)]
                cases = {"a": Case(c["shapes"], rank, c["mcr"], dev), "c": Case(c["shapes"], rank, c["mcr"], dev),
                         "d": Sequence(c["shapes"], rank, c["mcr"], dev)}
                try:
                    cases["b"] = Case(c["shapes"], rank, c["mcr"], dev, fused=True)
                except (TypeError, RuntimeError, ValueError):
                    pass  # this torch has no fused SGD
                cases = dict(sorted(cases.items()))

                def step(k, case):
                    x = cases[k]
                    grads = sets[case % nsets]
                    x.point(grads)
                    if k == "c":
                        sgd_step(x.opt, x.agg)
                    elif k == "d":
                        x.step(grads)
                    else:
                        optimizer_step(x.opt, x.agg)

                for k in cases:
                    for i in range(a.warmup):
                        step(k, i)
                one_call = sgd_step_applies(cases["c"].opt, cases["c"].agg)
                torch.cuda.synchronize()
                ms = {k: [] for k in cases}
                for _ in range(a.rounds):
                    for k in cases:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(a.steps):
                            step(k, i)
                        e1.record()
                        e1.synchronize()
                        ms[k].append(e0.elapsed_time(e1) / a.steps)
                med = {k: statistics.median(v) for k, v in ms.items()}
                out = {"shapes": name, "rank": rank, "iters": 2, "cache": cache, "steps": a.steps, "rounds": a.rounds,
                       "sgd_step_one_call": bool(one_call),
                       "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
                       "c_minus_a_ms": med["c"] - med["a"], "c_minus_b_ms": med["c"] - med["b"] if "b" in med else None,
                       "d_minus_a_ms": med["d"] - med["a"]}
                lines.append(json.dumps(out))
                print(lines[-1], flush=True)
                del cases, sets
                torch.cuda.empty_cache()
        if a.ulp:
            lines.append(json.dumps({"max_ulp_sgd_step_vs_torch_cfg3": ulp_distance(dev)}))
            print(lines[-1], flush=True)
    finally:
        torch.distributed.destroy_process_group()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
