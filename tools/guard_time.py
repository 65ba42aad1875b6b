"""What ``skip_nonfinite=True`` costs per step at world size 1 when every step is finite, the
alternatives interleaved in one run.

    python tools/guard_time.py [--configs cfg2_resnet50_r1 cfg3_resnet50_r4] [--steps 100] [--warmup 10]
                               [--rounds 7] [--parent-tree DIR]

Cases (each its own aggregator over the same shapes, the same rotating gradient sets: four sets of
ResNet-50 gradients are 400 MB, so every step reads its gradients cold):
  parent  the parent commit's step: a child process that imports ``powersgd_amd`` from DIR (a
          checkout of the parent commit with its library built) and times the same loop, one round
          at a time when this process asks for it (so the rounds of the two interleave and the two
          never time at once); left out without --parent-tree
  off     this commit's step, the guard off                  (the parent's code path)
  on      skip_nonfinite=True, every step finite             (two launches that write nothing)
  clip    max_grad_norm set, threshold never reached         (the clip's no-clip overhead, for scale)
  both    max_grad_norm and skip_nonfinite
Every round times `steps` calls of each case between two device events, in that order; the report
is the per-step median, min and max over the rounds and the differences the acceptance asks for,
with the run-to-run spread of `off` (max - min over the rounds) beside them. One JSON line per config."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1e30  # a threshold N(0, 1) gradients never reach


def _import(tree):
    if tree not in sys.path:
        sys.path.insert(0, tree)
    import torch
    from powersgd_amd import Config, PowerSGD
    from powersgd_amd.workloads import CONFIGS, hash_tensors
    return torch, Config, PowerSGD, CONFIGS, hash_tensors


class Bench:
    """One config's gradient sets and aggregators in this process."""

    def __init__(self, tree, name, cases, nsets, warmup):
        self.torch, Config, PowerSGD, CONFIGS, hash_tensors = _import(tree)
        torch = self.torch
        c = CONFIGS[name]
        dev = torch.device("cuda:0")
        dtype = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
        self.sets = [[torch.from_numpy(x).to(dev, dtype) for x in hash_tensors(c["shapes"], seed=11 + k)]
                     for k in range(nsets)]
        kw = {"parent": {}, "off": {}, "on": {"skip_nonfinite": True}, "clip": {"max_grad_norm": BIG},
              "both": {"max_grad_norm": BIG, "skip_nonfinite": True}}
        self.agg = {k: PowerSGD([torch.zeros(s, device=dev, dtype=dtype) for s in c["shapes"]],
                                Config(c["rank"], c["mcr"], c["iters"], 0), **kw[k]) for k in cases}
        for case in cases:
            self.run(case, warmup)
        torch.cuda.synchronize()

    def run(self, case, steps):
        for k in range(steps):
            self.agg[case].aggregate(self.sets[k % len(self.sets)])

    def time(self, case, steps):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(case, steps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps


def child(a):
    """The parent commit's side: per line on stdin `<config>` builds, `go` times one round."""
    bench = None
    for line in sys.stdin:
        word = line.strip()
        if word == "go":
            print(json.dumps(bench.time("parent", a.steps)), flush=True)
        elif word:
            bench = Bench(a.child, word, ["parent"], a.sets, a.warmup)
            print(json.dumps("ready"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg2_resnet50_r1", "cfg3_resnet50_r4"])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sets", type=int, default=4, help="gradient sets rotated by every case")
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
                                 "--steps", str(a.steps), "--warmup", str(a.warmup), "--sets", str(a.sets)],
                                stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)

    def ask(word):
        proc.stdin.write(word + "\n")
        proc.stdin.flush()
        line = proc.stdout.readline()
        if not line:
            raise RuntimeError("the parent-tree child ended")
        return json.loads(line)

    cases = ["off", "on", "clip", "both"]
    try:
        for name in a.configs:
            if proc:
                ask(name)
            bench = Bench(REPO, name, cases, a.sets, a.warmup)
            ms = {k: [] for k in (["parent"] if proc else []) + cases}
            for _ in range(a.rounds):
                if proc:
                    ms["parent"].append(ask("go"))
                for case in cases:
                    ms[case].append(bench.time(case, a.steps))
            med = {k: statistics.median(v) for k, v in ms.items()}
            out = {"config": name, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                   "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
                   "off_spread_ms": max(ms["off"]) - min(ms["off"]),
                   "on_minus_off_ms": med["on"] - med["off"], "clip_minus_off_ms": med["clip"] - med["off"],
                   "both_minus_clip_ms": med["both"] - med["clip"],
                   "skipped_steps_on": int(bench.agg["on"].skipped_steps)}
            if proc:
                out["off_minus_parent_ms"] = med["off"] - med["parent"]
            print(json.dumps(out), flush=True)
            del bench
    finally:
        if proc:
            proc.stdin.close()
            proc.wait(timeout=60)


if __name__ == "__main__":
    main()
