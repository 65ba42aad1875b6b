"""What one training step's communication + AdamW half costs at ranks 64 and 128, the alternatives
interleaved in one process.

    python tools/adam_wide_time.py [--steps 20] [--warmup 4] [--rounds 7] [--out profiles/adam_wide/adam_wide_time.jsonl]

One GPU, a one-rank process group over the library's communicator (the transport ``adam_step`` and
``adam_master_step`` serve). Shapes: ResNet-50 (two iterations per step) and the Llama-7B layer shapes
(one iteration), each at ranks 64 and 128, in both forms: "f32" (fp32 model, ``adam_step``) and "master"
(bf16 model and gradients, fp32 masters and moments, ``adam_master_step``). Cases (each its own parameters,
optimizer and aggregator over the same shapes and gradient sets; ``torch.optim.AdamW(lr=1e-3,
weight_decay=1e-2)``):
  a  the unfused sequence with torch's default AdamW (foreach): ``optimizer_step``, or aggregate_fp32 + the
     averages as the masters' .grad + optimizer.step() + model.copy_(master). This is what ``adam_step`` /
     ``adam_master_step`` did at these ranks before the wide entries existed
  b  the same with AdamW(fused=True)
  c  the one-call form (psgd_aggregate_comm_adam_wide / psgd_aggregate_mixed_comm_adam_wide)
Every step first hands over the next gradient set: "f32" points p.grad at it (the residual then replaces
it, as in tools/adam_step_time.py), "master" copies it into the model's .grad (consumed by the step, so
each step refills it); the same work in every case. Two passes per row: the sets rotated, so a step's gradients are
not the ones just read ("rotated"), and one set only ("same": everything warm). Every round times `steps`
steps of each case between two device events, in the order a, b, c. The report is the per-step median,
min and max over the rounds; a difference counts only beyond the spread (max - min) of both cases. One
JSON line per row and pass."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from powersgd_amd import (Config, Fp32ResidualPowerSGD, PowerSGD, adam_master_step, adam_master_step_applies,  # noqa: E402
                          adam_step, adam_step_applies, optimizer_step)
from powersgd_amd.workloads import CONFIGS, hash_tensors  # noqa: E402

HP = dict(lr=1e-3, weight_decay=1e-2)
ROWS = [(name, rank, form) for name in ("cfg3_resnet50_r4", "cfg4_llama_r2_bf16") for rank in (64, 128)
        for form in ("f32", "master")]


class Case:
    def __init__(self, shapes, rank, mcr, iters, dev, master, **opt_kw):
        gen = torch.Generator().manual_seed(5)
        self.master = master
        self.params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
        self.model = [torch.nn.Parameter(p.detach().bfloat16()) for p in self.params] if master else self.params
        for w in self.model:
            w.grad = torch.zeros_like(w)
        self.opt = torch.optim.AdamW(self.params, **HP, **opt_kw)
        self.agg = (Fp32ResidualPowerSGD if master else PowerSGD)(self.model, Config(rank, mcr, iters, 0))

    def applies(self):
        if self.master:
            return adam_master_step_applies(self.opt, self.agg, self.model)
        return adam_step_applies(self.opt, self.agg)

    def step(self, grads, one_call):
        if not self.master:  # as tools/adam_step_time.py: p.grad points at the set, the residual replaces it
            for p, g in zip(self.params, grads):
                p.grad = g
            return (adam_step if one_call else optimizer_step)(self.opt, self.agg)
        torch._foreach_copy_([w.grad for w in self.model], grads)
        if one_call:
            return adam_master_step(self.opt, self.agg, self.model)
        for p, a in zip(self.params, self.agg.aggregate_fp32([w.grad for w in self.model])):
            p.grad = a
        self.opt.step()
        with torch.no_grad():
            torch._foreach_copy_([w.data for w in self.model], [p.data for p in self.params])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    store = os.path.join(tempfile.mkdtemp(), "init")
    torch.distributed.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1, device_id=dev)
    lines = []
    try:
        for name, rank, form in ROWS:
            c = CONFIGS[name]
            master = form == "master"
            sets = [[torch.from_numpy(x).to(dev).to(torch.bfloat16 if master else torch.float32)
                     for x in hash_tensors(c["shapes"], seed=11 + k)] for k in range(3)]
            make = lambda **kw: Case(c["shapes"], rank, c["mcr"], c["iters"], dev, master, **kw)  # noqa: E731
            cases = {"a": make(), "b": make(fused=True), "c": make()}
            for k, x in cases.items():
                for i in range(a.warmup):
                    x.step(sets[i % 3], k == "c")
            one_call = cases["c"].applies()
            for label, nsets in (("rotated", 3), ("same", 1)):
                torch.cuda.synchronize()
                ms = {k: [] for k in cases}
                for _ in range(a.rounds):
                    for k, x in cases.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(a.steps):
                            x.step(sets[i % nsets], k == "c")
                        e1.record()
                        e1.synchronize()
                        ms[k].append(e0.elapsed_time(e1) / a.steps)
                med = {k: statistics.median(v) for k, v in ms.items()}
                out = {"shapes": name, "rank": rank, "iters": c["iters"], "form": form, "pass": label, "steps": a.steps,
                       "rounds": a.rounds, "one_call": bool(one_call),
                       "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
                       "c_minus_a_ms": med["c"] - med["a"], "c_minus_b_ms": med["c"] - med["b"]}
                lines.append(json.dumps(out))
                print(lines[-1], flush=True)
                if a.out:  # after every row: a run cut short keeps what it measured
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        f.write("\n".join(lines) + "\n")
            del cases, sets
            torch.cuda.empty_cache()
    finally:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
