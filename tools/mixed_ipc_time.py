"""Interleaved A/B of ``Fp32ResidualPowerSGD.aggregate`` under ``PSGD_COMM=ipc``: ``fused=True``
(psgd_aggregate_mixed_ipc: the bf16 averages written by the output pass, the uncompressed tensors'
by the last exchange) against ``fused=False`` (run-table ADD, psgd_aggregate_ipc on the fp32
residual, run-table GATHER), with W processes on ONE GPU, in the style of tools/mixed_comm_time.py.

Every process holds both aggregators (two exchange sessions) and feeds them its own bf16 gradients
(seeded by rank; re-filled before every timed call by a device copy outside the timed span:
``aggregate`` consumes them). Rounds rotate the order of the flows, the same order on every rank; a
host barrier outside the timed span lines the ranks up before each call; every call is timed alone
with HIP events around it on the codec's stream. The report is per rank and flow the median, the
quartiles and the spread (how far the medians of consecutive blocks of 20 calls move: max - min).
The yardstick is the unfused flow in the same process; the fused step counts as faster only when
its median beats the unfused median by more than the unfused spread.

One GPU, W processes: the exchange's loads and flags stay on the device, the processes' kernels
share its CUs. No cross-GPU traffic is measured.

usage: python tools/mixed_ipc_time.py [--world W] [--rounds N] [--warmup N] [--rank R] [--out FILE] [workload ...]
workloads: cfg4 (the cfg4_llama_r2_bf16 shapes, rank 2, one iteration; no uncompressed tensor) and
resnet50 (ResNet-50 shapes, rank 2, two iterations, bf16; its 1-D tensors are the flat tail); cfg4
by default."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": round(statistics.median(xs), 5), "q1_ms": round(q[0], 5), "q3_ms": round(q[2], 5),
            "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5)}


def run(name, w, a, rank_id):
    if a.rank is not None:
        w = dict(w, rank=a.rank)
    from powersgd_amd import Config, Fp32ResidualPowerSGD

    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    cfg = Config(w["rank"], w["mcr"], w["iters"], 0)
    gen = torch.Generator(device=dev).manual_seed(11 + 17 * rank_id)
    master = [torch.randn(s, generator=gen, device=dev).to(bf16) for s in w["shapes"]]
    keys = ("unfused", "fused")
    flows = {}
    for key in keys:
        agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=bf16, device=dev) for s in w["shapes"]], cfg,
                                   fused=key == "fused")
        flows[key] = dict(agg=agg, grads=[torch.empty_like(m) for m in master], times=[], folds=[])
    stream = torch.cuda.current_stream(dev)

    def one(key):
        f = flows[key]
        torch._foreach_copy_(f["grads"], master)  # refill (consumed by the previous call); not timed
        folds = f["agg"].fused_folds()
        torch.cuda.synchronize()
        torch.distributed.barrier()  # the ranks start the call together; not timed
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f["agg"].aggregate(f["grads"])
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), folds

    for r in range(a.warmup + a.rounds):
        order = keys[r % 2:] + keys[:r % 2]  # rotate who goes first, the same on every rank
        for key in order:
            ms, folds = one(key)
            if r >= a.warmup:
                flows[key]["times"].append(ms)
                flows[key]["folds"].append(folds)
    res = {"workload": name, "rank": w["rank"], "iters": w["iters"], "min_compression_rate": w["mcr"],
           "uncompressed_tensors": sum(not c for c in flows["fused"]["agg"].is_compressed_mask),
           "rounds": a.rounds, "warmup_rounds": a.warmup, "world": a.world, "process_rank": rank_id,
           "timed": "HIP events around each aggregate call, rotating order, ranks lined up by a host barrier"}
    for key, f in flows.items():
        t = f["times"]
        r = quartiles(t)
        blocks = [statistics.median(t[i:i + 20]) for i in range(0, len(t) - 19, 20)] or [r["median_ms"]]
        r["block_medians_spread_ms"] = round(max(blocks) - min(blocks), 5)
        r["folds_seen"] = sorted({tuple(x) for x in f["folds"]})
        res[key] = r
        timed_out = f["agg"].inner._powersgd.ipc_status()
        f["agg"].close()
        if timed_out:
            raise RuntimeError("an exchange wait timed out: the timings are void")
    gain = res["unfused"]["median_ms"] - res["fused"]["median_ms"]
    res["gain_ms"] = round(gain, 5)
    res["fused_beats_unfused_by_more_than_its_spread"] = bool(gain > res["unfused"]["block_medians_spread_ms"])
    return res


def worker(rank_id, a, initfile, outdir):
    os.environ["PSGD_COMM"] = "ipc"
    from powersgd_amd.workloads import CONFIGS, resnet50_shapes

    c4 = CONFIGS["cfg4_llama_r2_bf16"]
    workloads = {"cfg4": dict(shapes=c4["shapes"], rank=c4["rank"], iters=c4["iters"], mcr=c4["mcr"]),
                 "resnet50": dict(shapes=resnet50_shapes(), rank=2, iters=2, mcr=2)}
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=a.world)
    try:
        out = [run(n, workloads[n], a, rank_id) for n in a.workloads]
        with open(os.path.join(outdir, f"rank{rank_id}.json"), "w") as fh:
            json.dump(out, fh)
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rank", type=int, default=None, help="the workloads at this rank instead of their own")
    ap.add_argument("--out", default=None)
    ap.add_argument("workloads", nargs="*", default=["cfg4"])
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(worker, args=(a, os.path.join(td, "init"), td), nprocs=a.world, join=True)
        per_rank = [json.load(open(os.path.join(td, f"rank{r}.json"))) for r in range(a.world)]
    out = {"tool": "tools/mixed_ipc_time.py", "transport": "PSGD_COMM=ipc, %d processes on one GPU" % a.world,
           "results": [r for ranks in zip(*per_rank) for r in ranks]}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
