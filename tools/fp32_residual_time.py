"""Interleaved A/B of ``Fp32ResidualPowerSGD.aggregate`` with ``fused=True`` (psgd_aggregate_mixed:
the bf16 averages written, and where it pays the bf16 gradients ingested, by the codec's own passes) against
``fused=False`` (run-table ADD, fp32 codec, run-table GATHER), in ONE process on one GPU, and
against the fused call without its ingest fold (``fused_out_only``), so that each fold's gain
can be read on its own.

Both aggregators live side by side and take the same bf16 gradients (re-filled before every timed
call by a device copy outside the timed span: ``aggregate`` consumes them). Rounds rotate the
order of the flows, every call is timed alone with HIP events around it on the codec's stream,
and the report is per flow the median, the quartiles and the spread (how far the medians of
consecutive blocks of 20 calls move over the timed run: max - min), after a warm-up that covers
both step parities of both flows. The yardstick is the unfused flow in the same process; the
fused step counts as faster only when its median beats the unfused median by more than the
unfused spread. ``by_step_parity`` splits every flow by the codec step's parity, with the folds it
took there: where the parities fold differently (resnet50_i1: both folds on odd steps, the output
fold alone on even ones) the gain of each fold can be read against its separate pass.

usage: python tools/fp32_residual_time.py [--rounds N] [--warmup N] [--rank R] [--out FILE] [workload ...]
--rank R: the workloads at rank R instead of their own (16 / 32: the matrix-core final pass, which
has no ingest fold, so there ``fused_out_only`` is the same flow as ``fused``: an A/A control).
workloads: cfg4 (the cfg4_llama_r2_bf16 shapes), resnet50 (ResNet-50 shapes, rank 2, two
iterations, bf16) and resnet50_i1 (the same with one iteration per step), all by default."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from powersgd_amd import Config, Fp32ResidualPowerSGD  # noqa: E402
from powersgd_amd.workloads import CONFIGS, resnet50_shapes  # noqa: E402

WORKLOADS = {
    "cfg4": dict(shapes=CONFIGS["cfg4_llama_r2_bf16"]["shapes"], rank=CONFIGS["cfg4_llama_r2_bf16"]["rank"],
                 iters=CONFIGS["cfg4_llama_r2_bf16"]["iters"], mcr=CONFIGS["cfg4_llama_r2_bf16"]["mcr"]),
    "resnet50": dict(shapes=resnet50_shapes(), rank=2, iters=2, mcr=2),
    # one iteration per step: odd steps are the single-pass final kernel (the ingest fold's home)
    "resnet50_i1": dict(shapes=resnet50_shapes(), rank=2, iters=1, mcr=2),
}


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": round(statistics.median(xs), 5), "q1_ms": round(q[0], 5), "q3_ms": round(q[2], 5),
            "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5)}


def run(name, rounds, warmup, rank=None):
    w = dict(WORKLOADS[name], **({} if rank is None else {"rank": rank}))
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    cfg = Config(w["rank"], w["mcr"], w["iters"], 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    master = [torch.randn(s, generator=gen, device=dev).to(bf16) for s in w["shapes"]]
    flows = {}
    parity = {"unfused": [], "fused": [], "fused_out_only": []}
    # fused_out_only: the fused call with the ingest fold switched off (PSGD_MIXED_INGEST=0, read when
    # the plan is created): the library launches the run-table ADD itself, only the output folds
    for key, fused in (("unfused", False), ("fused", True), ("fused_out_only", True)):
        os.environ["PSGD_MIXED_INGEST"] = "0" if key == "fused_out_only" else "1"
        agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=bf16, device=dev) for s in w["shapes"]], cfg, fused=fused)
        os.environ.pop("PSGD_MIXED_INGEST")
        flows[key] = dict(agg=agg, grads=[torch.empty_like(m) for m in master], times=[], folds=[])
    stream = torch.cuda.current_stream(dev)

    def one(key):
        f = flows[key]
        torch._foreach_copy_(f["grads"], master)  # refill (consumed by the previous call); not timed
        folds = f["agg"].fused_folds()
        step = f["agg"].inner._powersgd.step_counter
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f["agg"].aggregate(f["grads"])
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), folds, step % 2

    for r in range(warmup + rounds):
        order = ("unfused", "fused", "fused_out_only")
        order = order[r % 3:] + order[:r % 3]  # rotate who goes first
        for key in order:
            ms, folds, par = one(key)
            if r >= warmup:
                flows[key]["times"].append(ms)
                flows[key]["folds"].append(folds)
                parity[key].append(par)
    res = {"workload": name, "rank": w["rank"], "iters": w["iters"], "min_compression_rate": w["mcr"],
           "rounds": rounds, "warmup_rounds": warmup, "timed": "HIP events around each aggregate call, rotating order"}
    for key, f in flows.items():
        t = f["times"]
        r = quartiles(t)
        # spread: how far the medians of consecutive blocks of 20 calls move (run-to-run noise of
        # the median itself), over the whole timed run
        blocks = [statistics.median(t[i:i + 20]) for i in range(0, len(t) - 19, 20)] or [r["median_ms"]]
        r["block_medians_spread_ms"] = round(max(blocks) - min(blocks), 5)
        r["folds_seen"] = sorted({tuple(x) for x in f["folds"]})
        r["by_step_parity"] = {
            ("even", "odd")[p]: {"median_ms": round(statistics.median([x for x, q in zip(t, parity[key]) if q == p]), 5),
                                 "folds": sorted({tuple(x) for x, q in zip(f["folds"], parity[key]) if q == p})}
            for p in sorted(set(parity[key]))}
        res[key] = r
        f["agg"].close()
    gain = res["unfused"]["median_ms"] - res["fused"]["median_ms"]
    res["gain_ms"] = round(gain, 5)
    res["fused_beats_unfused_by_more_than_its_spread"] = bool(gain > res["unfused"]["block_medians_spread_ms"])
    res["ingest_fold_gain_ms"] = round(res["fused_out_only"]["median_ms"] - res["fused"]["median_ms"], 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rank", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("workloads", nargs="*", default=list(WORKLOADS))
    a = ap.parse_args()
    out = {"tool": "tools/fp32_residual_time.py", "device": torch.cuda.get_device_name(0),
           "results": [run(n, a.rounds, a.warmup, a.rank) for n in a.workloads]}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
