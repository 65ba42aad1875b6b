"""What one training step's communication + SGD half costs at ranks 64 and 128, the alternatives interleaved.

    python tools/sgd_wide_time.py [--steps 20] [--warmup 4] [--rounds 7] [--parent-tree DIR]
                                  [--out profiles/sgd_wide/sgd_wide_time.jsonl]

One GPU, a one-rank process group over the library's communicator (the transport ``sgd_step`` serves). Shapes:
ResNet-50 (two iterations per step) and the Llama-7B layer shapes (one iteration), each at ranks 64 and 128, with
``torch.optim.SGD(lr=0.1, weight_decay=5e-4)`` at momentum 0.9 and at momentum 0 (no buffer: the final pass moves p
alone). Cases (each its own parameters, optimizer and aggregator over the same shapes and gradient sets):
  parent  the parent commit's ``sgd_step``, which at these ranks IS ``optimizer_step``: a child process that imports
          ``powersgd_amd`` from DIR (a checkout of the parent commit with its library built) and times the same loop,
          one round per request (the two processes never time at once); left out without --parent-tree
  a       ``optimizer_step`` with torch's default SGD (foreach): the same unfused sequence on this commit's library
  b       the same with SGD(fused=True)
  c       the one-call form (``sgd_step``: psgd_aggregate_comm_sgd_wide)
Every step first points p.grad at the next of three gradient sets (the residual then replaces it, as in
tools/sgd_step_time.py), so a step's gradients are not the ones just read. Every round times `steps` steps of each
case between two device events, in the order parent, a, b, c. The report is the per-step median, min and max over the
rounds; a difference counts only beyond the spread (max - min) of both cases. One JSON line per row."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(name, rank, mom) for name in ("cfg3_resnet50_r4", "cfg4_llama_r2_bf16") for rank in (64, 128)
        for mom in (0.9, 0.0)]


class Bench:
    """One row's gradient sets and cases in this process, `tree`'s package."""

    def __init__(self, tree, name, rank, mom, cases, warmup):
        if tree not in sys.path:
            sys.path.insert(0, tree)
        import torch
        from powersgd_amd import Config, PowerSGD, optimizer_step, sgd_step, sgd_step_applies
        from powersgd_amd.workloads import CONFIGS, hash_tensors

        self.torch = torch
        dev = torch.device("cuda:0")
        if not torch.distributed.is_initialized():
            torch.cuda.set_device(dev)
            store = os.path.join(tempfile.mkdtemp(), "init")
            torch.distributed.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1, device_id=dev)
        c = CONFIGS[name]
        self.iters = c["iters"]
        self.sets = [[torch.from_numpy(x).to(dev) for x in hash_tensors(c["shapes"], seed=11 + k)] for k in range(3)]
        self.case = {}
        for k in cases:
            gen = torch.Generator().manual_seed(5)
            params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in c["shapes"]]
            opt = torch.optim.SGD(params, lr=0.1, momentum=mom, weight_decay=5e-4, **({"fused": True} if k == "b" else {}))
            agg = PowerSGD(params, Config(rank, c["mcr"], c["iters"], 0))
            self.case[k] = (params, opt, agg, optimizer_step if k in "ab" else sgd_step)
        for k in cases:
            self.run(k, warmup)
        torch.cuda.synchronize()
        self.one_call = {k: bool(sgd_step_applies(o, g)) for k, (_, o, g, _) in self.case.items()}

    def run(self, k, steps):
        params, opt, agg, step = self.case[k]
        for i in range(steps):
            for p, g in zip(params, self.sets[i % 3]):
                p.grad = g
            step(opt, agg)

    def time(self, k, steps):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(k, steps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps


def child(a):
    """The parent commit's side: per line on stdin `<row>` builds, `go` times one round; replies are "@" + JSON."""
    bench = None
    for line in sys.stdin:
        word = line.strip()
        if word == "go":
            print("@" + json.dumps(bench.time("parent", a.steps)), flush=True)
        elif word:
            name, rank, mom = json.loads(word)
            bench = None  # the row before goes first
            bench = Bench(a.child, name, rank, mom, ["parent"], a.warmup)
            print("@" + json.dumps("ready"), flush=True)
    if bench is not None:
        bench.torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    proc = None
    if a.parent_tree:
        env = dict(os.environ)
        env.pop("PSGD_LIB_PATH", None)
        proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(a.parent_tree),
                                 "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)

    def ask(word):
        proc.stdin.write(word + "\n")
        proc.stdin.flush()
        while True:  # the child's replies start with "@"; the runtime may print lines of its own
            line = proc.stdout.readline()
            if not line:
                raise RuntimeError("the parent-tree child ended")
            if line.startswith("@"):
                return json.loads(line[1:])

    lines = []
    try:
        for name, rank, mom in ROWS:
            if proc:
                ask(json.dumps([name, rank, mom]))
            bench = Bench(REPO, name, rank, mom, ["a", "b", "c"], a.warmup)
            ms = {k: [] for k in (["parent"] if proc else []) + ["a", "b", "c"]}
            for _ in range(a.rounds):
                if proc:
                    ms["parent"].append(ask("go"))
                for k in "abc":
                    ms[k].append(bench.time(k, a.steps))
            med = {k: statistics.median(v) for k, v in ms.items()}
            out = {"shapes": name, "rank": rank, "iters": bench.iters, "momentum": mom, "steps": a.steps,
                   "rounds": a.rounds, "one_call": bench.one_call["c"],
                   "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
                   "c_minus_a_ms": med["c"] - med["a"], "c_minus_b_ms": med["c"] - med["b"]}
            if proc:
                out["a_minus_parent_ms"] = med["a"] - med["parent"]
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            if a.out:  # after every row: a run cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
            del bench
            import torch

            torch.cuda.empty_cache()
    finally:
        if proc:
            proc.stdin.close()
            proc.wait(timeout=60)
        import torch

        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
