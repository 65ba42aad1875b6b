"""Interleaved A/B of a wide-rank ``PowerSGD.aggregate`` step under ``PSGD_COMM=ipc``: every factor
exchange one-shot (``PSGD_IPC_TWO_SHOT=0``: k_xchg, each rank reads all W slots whole) against
two-shot (``PSGD_IPC_TWO_SHOT=1``: k_xchg_rs + k_xchg_ag, reduce-scatter + all-gather), in the
style of tools/mixed_ipc_time.py.

W processes, one per visible GPU where there are at least W, otherwise all on GPU 0; the output
names the topology it ran on. On ONE GPU the exchange's loads and flags stay on the device and the
processes' kernels share its CUs: such a run shows the launch and flag overhead of the second
launch only and says nothing about xGMI, where the two-shot form moves 2 (W - 1) / W of a factor
per rank instead of W - 1 times it.

Every process holds both codecs (two exchange sessions) and feeds them its own gradients (seeded by
rank; re-filled before every timed call by a device copy outside the timed span). Rounds rotate the
order of the two forms, the same order on every rank; a host barrier outside the timed span lines
the ranks up before each call; every call is timed alone with HIP events on the codec's stream. Per
rank and form: median, quartiles and the spread of the medians of consecutive blocks of 20 calls.

usage: python tools/ipc_two_shot_time.py [--world W] [--rounds N] [--warmup N] [--ranks 64 128]
           [--out FILE]
Workload: the matrices of ResNet-50, fp32, two power iterations, every matrix compressed."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FORMS = ("one_shot", "two_shot")


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": round(statistics.median(xs), 5), "q1_ms": round(q[0], 5), "q3_ms": round(q[2], 5),
            "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5)}


def run(rank, shapes, a, rank_id, dev):
    from powersgd_amd import Config, PowerSGD

    gen = torch.Generator(device=dev).manual_seed(11 + 17 * rank_id)
    master = [torch.randn(s, generator=gen, device=dev) for s in shapes]
    flows = {}
    for form in FORMS:
        os.environ["PSGD_IPC_TWO_SHOT"] = "1" if form == "two_shot" else "0"  # read at the session's setup
        psgd = PowerSGD([torch.zeros(s, device=dev) for s in shapes], Config(rank, 0, 2, 0))
        grads = [m.clone() for m in master]
        psgd.aggregate(grads)  # opens the session in this form
        plan = psgd._powersgd._plan
        assert plan.is_wide() and plan.ipc_two_shot(0) == plan.ipc_two_shot(1) == (form == "two_shot" and a.world > 1)
        flows[form] = dict(psgd=psgd, grads=grads, times=[])
    os.environ.pop("PSGD_IPC_TWO_SHOT", None)
    stream = torch.cuda.current_stream(dev)

    def one(form):
        f = flows[form]
        torch._foreach_copy_(f["grads"], master)  # refill (the call leaves the residual there); not timed
        torch.cuda.synchronize(dev)
        torch.distributed.barrier()  # the ranks start the call together; not timed
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f["psgd"].aggregate(f["grads"])
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for r in range(a.warmup + a.rounds):
        order = FORMS[r % 2:] + FORMS[:r % 2]  # rotate who goes first, the same on every rank
        for form in order:
            ms = one(form)
            if r >= a.warmup:
                flows[form]["times"].append(ms)
    pn, qn = flows["one_shot"]["psgd"]._powersgd._plan.factor_numel()
    res = {"workload": "resnet50 matrices, fp32", "rank": rank, "iters": 2, "world": a.world, "process_rank": rank_id,
           "p_factor_bytes": 4 * pn, "q_factor_bytes": 4 * qn, "rounds": a.rounds, "warmup_rounds": a.warmup,
           "timed": "HIP events around each aggregate call, rotating order, ranks lined up by a host barrier"}
    for form, f in flows.items():
        t = f["times"]
        r = quartiles(t)
        blocks = [statistics.median(t[i:i + 20]) for i in range(0, len(t) - 19, 20)] or [r["median_ms"]]
        r["block_medians_spread_ms"] = round(max(blocks) - min(blocks), 5)
        res[form] = r
        timed_out = f["psgd"]._powersgd.ipc_status()
        f["psgd"].close()
        if timed_out:
            raise RuntimeError("an exchange wait timed out: the timings are void")
    res["two_shot_minus_one_shot_ms"] = round(res["two_shot"]["median_ms"] - res["one_shot"]["median_ms"], 5)
    return res


def worker(rank_id, a, initfile, outdir, one_per_gpu):
    os.environ["PSGD_COMM"] = "ipc"
    from powersgd_amd.workloads import resnet50_shapes

    shapes = [s for s in resnet50_shapes() if len(s) > 1]
    dev = torch.device("cuda", rank_id if one_per_gpu else 0)
    torch.cuda.set_device(dev)
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=a.world)
    try:
        out = [run(r, shapes, a, rank_id, dev) for r in a.ranks]
        with open(os.path.join(outdir, f"rank{rank_id}.json"), "w") as fh:
            json.dump(out, fh)
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ranks", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ngpu = torch.cuda.device_count()
    one_per_gpu = ngpu >= a.world and a.world > 1
    topology = ("%d processes, one per GPU (%d visible)" % (a.world, ngpu) if one_per_gpu
                else "%d processes on ONE GPU: launch and flag overhead only, no cross-GPU traffic" % a.world)
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(worker, args=(a, os.path.join(td, "init"), td, one_per_gpu), nprocs=a.world,
                                    join=True)
        per_rank = [json.load(open(os.path.join(td, f"rank{r}.json"))) for r in range(a.world)]
    out = {"tool": "tools/ipc_two_shot_time.py", "transport": "PSGD_COMM=ipc", "topology": topology,
           "results": [r for ranks in zip(*per_rank) for r in ranks]}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
