"""Step time of PowerSGD.aggregate at ranks 32 / 64 / 128 (world size 1, two power iterations).

Times the rank-32 path and the wide-rank path (ranks 33-128, psgd_wide.hip) with one method in
one process: per case a warm-up, then event-timed ``aggregate`` steps over rotating gradient
sets (cold Infinity Cache, as bench.py times its headline). Workloads: the matrices of
ResNet-50 (``resnet50_shapes()`` without the 1-D tensors) and the cfg4 LLaMA matrices, fp32 and
bf16. One JSON per run goes to ``profiles/wide_rank/`` (or ``--out``).

For per-kernel times run it once under the profiler, as a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o wide -- \
      python tools/wide_rank_time.py --workloads resnet50 --dtypes f32 --steps 5 --warmup 2

usage: python tools/wide_rank_time.py [--steps 20] [--warmup 3] [--sets 3]
           [--ranks 32 64 128] [--workloads resnet50 llama] [--dtypes f32 bf16] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

from powersgd_amd import Config, PowerSGD  # noqa: E402
from powersgd_amd.workloads import CONFIGS, hash_tensors, resnet50_shapes  # noqa: E402

WORKLOADS = {
    "resnet50": [s for s in resnet50_shapes() if len(s) > 1],
    "llama": list(CONFIGS["cfg4_llama_r2_bf16"]["shapes"]),
}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def time_case(shapes, rank, dtype, steps, warmup, nsets, dev):
    psgd = PowerSGD([torch.zeros(s, device=dev, dtype=dtype) for s in shapes], Config(rank, 0, 2, 0))
    assert all(psgd.is_compressed_mask)
    base = [[torch.from_numpy(f).to(dev).to(dtype) for f in hash_tensors(shapes, seed=40 + k)] for k in range(nsets)]
    sets = [[g.clone() for g in b] for b in base]

    def refill():  # the residual left in a set must not accumulate over the run
        for s, b in zip(sets, base):
            for x, y in zip(s, b):
                x.copy_(y)

    for k in range(warmup):
        psgd.aggregate(sets[k % nsets])
    refill()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for k in range(steps):
        evs[k][0].record()
        psgd.aggregate(sets[k % nsets])
        evs[k][1].record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    return {"rank": rank, "wide": bool(psgd._powersgd._plan.is_wide()), "ms_median": statistics.median(ms),
            "ms_min": min(ms), "ms_max": max(ms), "steps": steps, "gradient_bytes": numel * (4 if dtype == torch.float32 else 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--ranks", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--workloads", nargs="+", default=sorted(WORKLOADS), choices=sorted(WORKLOADS))
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=sorted(DTYPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_rank"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "iters": 2, "world": 1, "cache": "cold", "sets": a.sets,
              "cases": []}
    for w in a.workloads:
        for d in a.dtypes:
            base_ms = None
            for rank in a.ranks:
                c = time_case(WORKLOADS[w], rank, DTYPES[d], a.steps, a.warmup, a.sets, dev)
                c.update(workload=w, dtype=d)
                if rank == 32:
                    base_ms = c["ms_median"]
                if base_ms:
                    c["vs_rank32"] = c["ms_median"] / base_ms
                result["cases"].append(c)
                print(json.dumps(c), flush=True)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, time.strftime("wide_rank_%Y%m%d_%H%M%S.json"))
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
