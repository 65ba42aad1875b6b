"""What one training step's communication + SGD half costs for a bf16 model with fp32 master weights,
the alternatives interleaved in one process.

    python tools/sgd_master_time.py [--steps 20] [--warmup 5] [--rounds 7] [--out profiles/sgd_master/sgd_master_time.jsonl]

One GPU, a one-rank process group over the library's communicator (the transport ``sgd_master_step``
serves). Shapes: ResNet-50 (two iterations per step) and the Llama-7B layer shapes (one iteration) at
ranks 1, 4, 16, 64 and 128, with momentum 0.9 and without; bf16 model and gradients, fp32 masters and
momentum buffers. Cases (each its own model, masters, optimizer and ``Fp32ResidualPowerSGD`` over the
same shapes and gradient sets; ``torch.optim.SGD(lr=0.1, weight_decay=5e-4)`` on the masters):
  a  the unfused sequence (aggregate_fp32, averages as the masters' .grad, optimizer.step(), model.copy_(master)),
     torch's default SGD (foreach)
  b  the same with SGD(fused=True)
  c  sgd_master_step in its one-call form             (psgd_aggregate_mixed_comm_sgd[_wide])
Every step first fills the model's .grad from the next of three gradient sets (the gradients are
consumed, so each step refills them: the same device work in every case; the sets rotate, so a step's
gradients are not the ones just read). Every round times `steps` steps of each case between two device
events, in the order a, b, c. The report is the per-step median, min and max over the rounds; a
difference counts only beyond the spread (max - min) of both cases. One JSON line per row."""
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

from powersgd_amd import Config, Fp32ResidualPowerSGD, sgd_master_step, sgd_master_step_applies  # noqa: E402
from powersgd_amd.workloads import CONFIGS, hash_tensors  # noqa: E402

ROWS = [(name, rank, mom) for name in ("cfg3_resnet50_r4", "cfg4_llama_r2_bf16") for rank in (1, 4, 16, 64, 128)
        for mom in (0.9, 0.0)]


class Case:
    def __init__(self, shapes, rank, mcr, iters, mom, dev, **opt_kw):
        gen = torch.Generator().manual_seed(5)
        self.masters = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
        self.model = [torch.nn.Parameter(p.detach().bfloat16()) for p in self.masters]
        for w in self.model:
            w.grad = torch.zeros_like(w)
        self.opt = torch.optim.SGD(self.masters, lr=0.1, momentum=mom, weight_decay=5e-4, **opt_kw)
        self.agg = Fp32ResidualPowerSGD(self.model, Config(rank, mcr, iters, 0))

    def step(self, grads, one_call):
        torch._foreach_copy_([w.grad for w in self.model], grads)
        if one_call:
            return sgd_master_step(self.opt, self.agg, self.model)
        for p, a in zip(self.masters, self.agg.aggregate_fp32([w.grad for w in self.model])):
            p.grad = a
        self.opt.step()
        with torch.no_grad():
            torch._foreach_copy_([w.data for w in self.model], [p.data for p in self.masters])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    store = os.path.join(tempfile.mkdtemp(), "init")
    torch.distributed.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1, device_id=dev)
    lines, sets, have = [], None, None
    try:
        for name, rank, mom in ROWS:
            c = CONFIGS[name]
            if have != name:
                sets = [[torch.from_numpy(x).to(dev).bfloat16() for x in hash_tensors(c["shapes"], seed=11 + k)] for k in range(3)]
                have = name
            make = lambda **kw: Case(c["shapes"], rank, c["mcr"], c["iters"], mom, dev, **kw)  # noqa: E731
            cases = {"a": make(), "b": make(fused=True), "c": make()}
            for k, x in cases.items():
                for i in range(a.warmup):
                    x.step(sets[i % 3], k == "c")
            one_call = sgd_master_step_applies(cases["c"].opt, cases["c"].agg, cases["c"].model)
            torch.cuda.synchronize()
            ms = {k: [] for k in cases}
            for _ in range(a.rounds):
                for k, x in cases.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(a.steps):
                        x.step(sets[i % 3], k == "c")
                    e1.record()
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1) / a.steps)
            med = {k: statistics.median(v) for k, v in ms.items()}
            out = {"shapes": name, "rank": rank, "iters": c["iters"], "momentum": mom, "model": "bf16", "masters": "f32",
                   "steps": a.steps, "rounds": a.rounds, "sgd_master_step_one_call": bool(one_call),
                   "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
                   "c_minus_a_ms": med["c"] - med["a"], "c_minus_b_ms": med["c"] - med["b"]}
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            del cases
            torch.cuda.empty_cache()
    finally:
        torch.distributed.destroy_process_group()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
