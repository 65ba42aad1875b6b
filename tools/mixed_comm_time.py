"""Interleaved A/B of ``Fp32ResidualPowerSGD.aggregate`` in a process group that runs over the
library's own communicator: ``fused=True`` (psgd_aggregate_mixed_comm: the bf16 averages written by
the final pass of the W > 1 sequence, the flat tail rounded in the same launch) against
``fused=False`` (run-table ADD, psgd_aggregate_comm on the fp32 residual, run-table GATHER), in ONE
process on one GPU, in the style of tools/fp32_residual_time.py.

Both aggregators live side by side and take the same bf16 gradients (re-filled before every timed
call by a device copy outside the timed span: ``aggregate`` consumes them). Rounds rotate the order
of the flows, every call is timed alone with HIP events around it on the codec's stream, and the
report is per flow the median, the quartiles and the spread (how far the medians of consecutive
blocks of 20 calls move over the timed run: max - min), after a warm-up that covers both step
parities of both flows. The yardstick is the unfused flow in the same process; the fused step counts
as faster only when its median beats the unfused median by more than the unfused spread.

--comm stub   the stand-in collective library of the tests (tests/stubs/librccl_stub.so, built by
              build()) at --world W: the W > 1 kernel instances run, a collective is a plain
              kernel on both sides. Test infrastructure: no cross-device traffic is measured.
--comm rccl   a real 1-rank RCCL group (torch.distributed backend nccl): the orchestration cost
              of the real library; the final pass is the world-size-1 instance.
--unfused-only  time the unfused flow alone (a build without the fused communicator call).

usage: python tools/mixed_comm_time.py --comm stub|rccl [--world W] [--rounds N] [--warmup N]
                                       [--rank R] [--unfused-only] [--out FILE] [workload ...]
workloads: cfg4 (the cfg4_llama_r2_bf16 shapes, rank 2, one iteration) and resnet50 (ResNet-50
shapes, rank 2, two iterations, bf16), both by default."""
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


def run(name, w, a):
    if a.rank is not None:
        w = dict(w, rank=a.rank)
    from powersgd_amd import Config, Fp32ResidualPowerSGD, _lib

    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    cfg = Config(w["rank"], w["mcr"], w["iters"], 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    master = [torch.randn(s, generator=gen, device=dev).to(bf16) for s in w["shapes"]]
    keys = ("unfused",) if a.unfused_only else ("unfused", "fused")
    flows = {}
    for key in keys:
        agg = Fp32ResidualPowerSGD([torch.zeros(s, dtype=bf16, device=dev) for s in w["shapes"]], cfg,
                                   fused=key == "fused")
        if a.comm == "stub":  # the library's communicator, created through the stand-in at world W
            agg.inner._powersgd._comm = _lib.Comm(a.world, 0, _lib.comm_unique_id(), 0)
        flows[key] = dict(agg=agg, grads=[torch.empty_like(m) for m in master], times=[], folds=[], parity=[])
    stream = torch.cuda.current_stream(dev)

    def one(key):
        f = flows[key]
        torch._foreach_copy_(f["grads"], master)  # refill (consumed by the previous call); not timed
        folds = f["agg"].fused_folds()
        step = f["agg"].inner._powersgd.step_counter
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f["agg"].aggregate(f["grads"])
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), folds, step % 2

    for r in range(a.warmup + a.rounds):
        order = keys[r % len(keys):] + keys[:r % len(keys)]  # rotate who goes first
        for key in order:
            ms, folds, par = one(key)
            if r >= a.warmup:
                flows[key]["times"].append(ms)
                flows[key]["folds"].append(folds)
                flows[key]["parity"].append(par)
    plan = flows["unfused"]["agg"].inner._powersgd._plan
    res = {"workload": name, "rank": w["rank"], "iters": w["iters"], "min_compression_rate": w["mcr"],
           "rounds": a.rounds, "warmup_rounds": a.warmup, "comm": a.comm,
           "world": a.world if a.comm == "stub" else 1,
           # the final pass of the W > 1 sequence by step parity: 1 = k_final_odd + the output pass
           "fused_final_by_step_parity": [plan.fused_final(0, False), plan.fused_final(1, False)],
           "timed": "HIP events around each aggregate call, rotating order"}
    for key, f in flows.items():
        t = f["times"]
        r = quartiles(t)
        blocks = [statistics.median(t[i:i + 20]) for i in range(0, len(t) - 19, 20)] or [r["median_ms"]]
        r["block_medians_spread_ms"] = round(max(blocks) - min(blocks), 5)
        r["folds_seen"] = sorted({tuple(x) for x in f["folds"]})
        r["by_step_parity"] = {
            ("even", "odd")[p]: {"median_ms": round(statistics.median([x for x, q in zip(t, f["parity"]) if q == p]), 5)}
            for p in sorted(set(f["parity"]))}
        res[key] = r
        f["agg"].close()
    if "fused" in res:
        gain = res["unfused"]["median_ms"] - res["fused"]["median_ms"]
        res["gain_ms"] = round(gain, 5)
        res["fused_beats_unfused_by_more_than_its_spread"] = bool(gain > res["unfused"]["block_medians_spread_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--comm", required=True, choices=["stub", "rccl"])
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--unfused-only", action="store_true")
    ap.add_argument("--rank", type=int, default=None, help="the workloads at this rank instead of their own")
    ap.add_argument("--out", default=None)
    ap.add_argument("workloads", nargs="*", default=["cfg4", "resnet50"])
    a = ap.parse_args()
    if a.comm == "stub":
        os.environ["PSGD_RCCL_LIB_FORCE"] = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
        os.environ["PSGD_TESTING"] = "1"
    from powersgd_amd.workloads import CONFIGS, resnet50_shapes

    c4 = CONFIGS["cfg4_llama_r2_bf16"]
    workloads = {"cfg4": dict(shapes=c4["shapes"], rank=c4["rank"], iters=c4["iters"], mcr=c4["mcr"]),
                 "resnet50": dict(shapes=resnet50_shapes(), rank=2, iters=2, mcr=2)}
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as td:
        # one rank: the group makes is_distributed() true (stub: gloo, the communicator is the
        # stand-in's; rccl: the library creates its own 1-rank communicator beside torch's)
        torch.distributed.init_process_group("gloo" if a.comm == "stub" else "nccl",
                                             init_method=f"file://{td}/store", rank=0, world_size=1)
        try:
            out = {"tool": "tools/mixed_comm_time.py", "device": torch.cuda.get_device_name(0),
                   "results": [run(n, workloads[n], a) for n in a.workloads]}
        finally:
            torch.distributed.destroy_process_group()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
