"""What global-norm clipping costs per step at world size 1, the alternatives interleaved in one process.

    python tools/clip_time.py [--configs cfg2_resnet50_r1 cfg3_resnet50_r4] [--steps 100] [--warmup 10] [--rounds 7]

Cases (each its own aggregator over the same shapes, the same rotating gradient sets):
  a  aggregate alone                                         (no clipping: the reference point)
  b  max_grad_norm set, factor form, threshold never reached (norm + a scale launch that exits)
  c  the same, threshold always exceeded                     (norm + the scale pass)
  d  stream form (PSGD_NORM_FORM=stream), always clipping
  e  aggregate, then torch.nn.utils.clip_grad_norm_ on the returned tensors, always clipping
  f  stream form, threshold never reached                    (against b: the two forms' norms alone)
Every round times `steps` calls of each case between two device events, in the order a..f; the
report is the per-step median, min and max over the rounds, and the differences and ratios the
acceptance asks for. One JSON line per config."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from powersgd_amd import Config, PowerSGD  # noqa: E402
from powersgd_amd.workloads import CONFIGS, hash_tensors  # noqa: E402

BIG, TINY = 1e30, 1e-12  # thresholds never / always exceeded by N(0, 1) gradients


def build(c, dev, dtype, env=None, **kw):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return PowerSGD([torch.zeros(s, device=dev, dtype=dtype) for s in c["shapes"]],
                        Config(c["rank"], c["mcr"], c["iters"], 0), **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg2_resnet50_r1", "cfg3_resnet50_r4"], choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sets", type=int, default=4, help="gradient sets rotated by every case")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.configs:
        c = CONFIGS[name]
        dtype = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
        sets = [[torch.from_numpy(x).to(dev, dtype) for x in hash_tensors(c["shapes"], seed=11 + k)]
                for k in range(a.sets)]
        params = [torch.nn.Parameter(torch.zeros(s, device=dev, dtype=dtype)) for s in c["shapes"]]
        agg = {"a": build(c, dev, dtype), "b": build(c, dev, dtype, max_grad_norm=BIG),
               "c": build(c, dev, dtype, max_grad_norm=TINY),
               "d": build(c, dev, dtype, env={"PSGD_NORM_FORM": "stream"}, max_grad_norm=TINY),
               "e": build(c, dev, dtype),
               "f": build(c, dev, dtype, env={"PSGD_NORM_FORM": "stream"}, max_grad_norm=BIG)}
        forms = {k: None for k in agg}

        def step(case, k):
            outs = agg[case].aggregate(sets[k % a.sets])
            if case == "e":
                for p, o in zip(params, outs):
                    p.grad = o
                torch.nn.utils.clip_grad_norm_(params, TINY, foreach=True)
            return outs

        for case in agg:
            for k in range(a.warmup):
                step(case, k)
            codec = agg[case]._powersgd
            forms[case] = codec._plan.norm_form(codec.step_counter - 1, 1)
        torch.cuda.synchronize()
        ms = {k: [] for k in agg}
        for _ in range(a.rounds):
            for case in agg:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(a.steps):
                    step(case, k)
                e1.record()
                e1.synchronize()
                ms[case].append(e0.elapsed_time(e1) / a.steps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        out = {"config": name, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
               "auto_form_after_step": forms,  # 1 factors, 2 stream
               "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
               "b_minus_a_ms": med["b"] - med["a"], "c_minus_a_ms": med["c"] - med["a"],
               "d_minus_a_ms": med["d"] - med["a"], "e_minus_a_ms": med["e"] - med["a"],
               "b_over_e": med["b"] / med["e"], "c_over_e": med["c"] / med["e"], "d_over_e": med["d"] / med["e"],
               "f_minus_a_ms": med["f"] - med["a"], "b_minus_f_ms": med["b"] - med["f"],
               "last_norm_b": float(agg["b"].last_grad_norm), "last_coef_c": float(agg["c"].last_clip_coef)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
