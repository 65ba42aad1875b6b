"""What one training step's communication + AdamW half costs for a bf16 model with fp32 master weights,
the alternatives interleaved in one process.

    python tools/adam_master_time.py [--steps 30] [--warmup 5] [--rounds 7] [--out profiles/adam_master/adam_master_time.jsonl]

One GPU, a one-rank process group over the library's communicator (the transport ``adam_master_step``
serves). Shapes: ResNet-50 at ranks 1, 4 and 16 (two iterations per step) and the Llama-7B layer shapes
at rank 2 (one iteration); bf16 model and gradients, fp32 masters and moments. Cases (each its own
model, masters, optimizer and ``Fp32ResidualPowerSGD`` over the same shapes and gradient sets;
``torch.optim.AdamW(lr=1e-3, weight_decay=1e-2)`` on the masters):
  a  the unfused sequence (aggregate_fp32, averages as the masters' .grad, optimizer.step(), model.copy_(master)),
     torch's default AdamW (foreach)
  b  the same with AdamW(fused=True)
  c  adam_master_step in its one-call form            (psgd_aggregate_mixed_comm_adam)
Every step first points the model's .grad at a copy target filled from the next gradient set (the
gradients are consumed, so each step refills them: the same device work in every case). Two passes per
row: the sets rotated, so a step's gradients are not the ones just read ("rotated"), and one set only
("same": everything warm). Every round times `steps` steps of each case between two device events, in
the order a, b, c. The report is the per-step median, min and max over the rounds; a difference counts
only beyond the spread (max - min) of both cases. One JSON line per row and pass."""
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

from powersgd_amd import Config, Fp32ResidualPowerSGD, adam_master_step, adam_master_step_applies  # noqa: E402
from powersgd_amd.workloads import CONFIGS, hash_tensors  # noqa: E402

HP = dict(lr=1e-3, weight_decay=1e-2)
ROWS = [("cfg2_resnet50_r1", 1), ("cfg3_resnet50_r4", 4), ("cfg3_resnet50_r4", 16), ("cfg4_llama_r2_bf16", 2)]


class Case:
    def __init__(self, shapes, rank, mcr, iters, dev, **opt_kw):
        gen = torch.Generator().manual_seed(5)
        self.masters = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
        self.model = [torch.nn.Parameter(p.detach().bfloat16()) for p in self.masters]
        for w in self.model:
            w.grad = torch.zeros_like(w)
        self.opt = torch.optim.AdamW(self.masters, **HP, **opt_kw)
        self.agg = Fp32ResidualPowerSGD(self.model, Config(rank, mcr, iters, 0))

    def step(self, grads, one_call):
        torch._foreach_copy_([w.grad for w in self.model], grads)
        if one_call:
            return adam_master_step(self.opt, self.agg, self.model)
        for p, a in zip(self.masters, self.agg.aggregate_fp32([w.grad for w in self.model])):
            p.grad = a
        self.opt.step()
        with torch.no_grad():
            torch._foreach_copy_([w.data for w in self.model], [p.data for p in self.masters])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    store = os.path.join(tempfile.mkdtemp(), "init")
    torch.distributed.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1, device_id=dev)
    lines = []
    try:
        for name, rank in ROWS:
            c = CONFIGS[name]
            sets = [[torch.from_numpy(x).to(dev).bfloat16() for x in hash_tensors(c["shapes"], seed=11 + k)] for k in range(3)]
            make = lambda **kw: Case(c["shapes"], rank, c["mcr"], c["iters"], dev, **kw)  # noqa: E731
            cases = {"a": make(), "b": make(fused=True), "c": make()}
            for k, x in cases.items():
                for i in range(a.warmup):
                    x.step(sets[i % 3], k == "c")
            one_call = adam_master_step_applies(cases["c"].opt, cases["c"].agg, cases["c"].model)
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
                out = {"shapes": name, "rank": rank, "iters": c["iters"], "model": "bf16", "masters": "f32", "pass": label,
                       "steps": a.steps, "rounds": a.rounds, "adam_master_step_one_call": bool(one_call),
                       "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
                       "c_minus_a_ms": med["c"] - med["a"], "c_minus_b_ms": med["c"] - med["b"]}
                lines.append(json.dumps(out))
                print(lines[-1], flush=True)
            del cases, sets
            torch.cuda.empty_cache()
    finally:
        torch.distributed.destroy_process_group()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
