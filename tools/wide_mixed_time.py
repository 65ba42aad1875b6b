"""Step time of Fp32ResidualPowerSGD.aggregate at ranks 64 / 128 (bf16 gradients, fp32 residual,
world size 1, two power iterations): fused=True (psgd_aggregate_mixed_wide, final pass
k_wide_apply_mix) against fused=False (run-table ADD, the fp32 wide codec, run-table GATHER).

Both aggregators live in one process and are timed interleaved: per round, `steps` event-timed
steps of one, then of the other, over rotating gradient sets (cold Infinity Cache, as bench.py
times its headline); `rounds` rounds give the run-to-run spread of each median. Workloads: the
matrices of ResNet-50 and the cfg4 LLaMA matrices. The result is written to
``profiles/wide_mixed/fused_ab.json`` (``--out DIR``: to DIR/fused_ab.json). The defaults time
8 x 40 steps per variant and case, 0.4-1.7 s of device work each.

usage: python tools/wide_mixed_time.py [--steps 40] [--warmup 3] [--rounds 8] [--sets 3]
           [--ranks 64 128] [--workloads resnet50 llama] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

from powersgd_amd import Config, Fp32ResidualPowerSGD  # noqa: E402
from powersgd_amd.workloads import CONFIGS, hash_tensors, resnet50_shapes  # noqa: E402

WORKLOADS = {
    "resnet50": [s for s in resnet50_shapes() if len(s) > 1],
    "llama": list(CONFIGS["cfg4_llama_r2_bf16"]["shapes"]),
}
BF16 = torch.bfloat16


def time_case(shapes, rank, steps, warmup, rounds, nsets, dev):
    aggs = {f: Fp32ResidualPowerSGD([torch.zeros(s, device=dev, dtype=BF16) for s in shapes], Config(rank, 0, 2, 0), fused=f)
            for f in (False, True)}
    assert aggs[True].fused_folds() == (0, 1) and aggs[False].fused_folds() == (0, 0)
    base = [[torch.from_numpy(f).to(dev).to(BF16) for f in hash_tensors(shapes, seed=40 + k)] for k in range(nsets)]
    sets = [[g.clone() for g in b] for b in base]

    def refill():  # the gradients are consumed (zeroed) by every step
        for s, b in zip(sets, base):
            for x, y in zip(s, b):
                x.copy_(y)

    def run(agg, n, timed):
        ms = []
        for k in range(n):
            if k % nsets == 0:
                refill()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            agg.aggregate(sets[k % nsets])
            b.record()
            ms.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ms] if timed else []

    for f in (False, True):
        run(aggs[f], warmup, False)
    med = {False: [], True: []}
    for _ in range(rounds):
        for f in (False, True):
            aggs[f].residual.zero_()  # bounded values over a long run
            med[f].append(statistics.median(run(aggs[f], steps, True)))
    out = {"rank": rank, "steps": steps, "rounds": rounds,
           "gradient_bytes": 2 * sum(int(torch.Size(s).numel()) for s in shapes)}
    for f, name in ((False, "three_stage"), (True, "fused")):
        out[name] = {"ms_median": statistics.median(med[f]), "ms_round_min": min(med[f]), "ms_round_max": max(med[f])}
    out["fused_over_three_stage"] = out["fused"]["ms_median"] / out["three_stage"]["ms_median"]
    out["spread_rel_max"] = max((out[n]["ms_round_max"] - out[n]["ms_round_min"]) / out[n]["ms_median"]
                                for n in ("three_stage", "fused"))
    for a in aggs.values():
        a.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--ranks", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--workloads", nargs="+", default=sorted(WORKLOADS), choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_mixed"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "iters": 2, "world": 1, "cache": "cold", "sets": a.sets, "cases": []}
    for w in a.workloads:
        for rank in a.ranks:
            c = time_case(WORKLOADS[w], rank, a.steps, a.warmup, a.rounds, a.sets, dev)
            c.update(workload=w)
            result["cases"].append(c)
            print(json.dumps(c), flush=True)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "fused_ab.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
