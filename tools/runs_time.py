"""Event-timed run-table passes: the same-dtype fp32 add / gather (k_runs<float>) against the
mixed add / gather (bf16 bucket side over fp32 tensors, psgd_runs_create_mixed) on one run per
parameter, the layout of the DDP hook's state (tensors: views of one flat fp32 buffer; bucket:
one flat buffer in parameter order).

Per workload (the ResNet-50 parameter list, the cfg4 LLaMA shapes) the four passes alternate in
one process after a warm-up; each launch is bracketed by its own pair of events. Reported per
pass: median, min, max and the inter-quartile range in microseconds, the bytes the pass has to
move and the rate at the median; and the mixed / fp32 ratio of the medians with the fp32 pass's
relative spread (IQR / median) beside it. Writes one JSON document to stdout (and to --out).
usage: python tools/runs_time.py [--reps 60] [--warmup 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from powersgd_amd import _lib  # noqa: E402
from powersgd_amd.workloads import CONFIGS  # noqa: E402

DEV = torch.device("cuda:0")
WORKLOADS = {"resnet50": CONFIGS["cfg2_resnet50_r1"]["shapes"], "cfg4_llama": CONFIGS["cfg4_llama_r2_bf16"]["shapes"]}
# bytes per element a pass has to move: add reads both sides and writes the tensors; gather
# reads the tensors and writes the bucket
BYTES = {"add_f32": 12, "add_mixed": 10, "gather_f32": 8, "gather_mixed": 6}


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def _table(numels, tcode, bcode):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += n
    runs = _lib.Runs(offs, list(range(len(numels))), [0] * len(numels), numels, len(numels), tcode, bcode)
    ws = torch.empty(runs.workspace_bytes(), dtype=torch.uint8, device=DEV)
    runs.bind(0, ws.data_ptr())
    return runs, ws


def _summary(us, bytes_moved):
    us = sorted(us)
    q = statistics.quantiles(us, n=4)
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
            "iqr_us": round(q[2] - q[0], 2), "rel_spread": round((q[2] - q[0]) / med, 4), "reps": len(us),
            "bytes": bytes_moved, "tb_per_s": round(bytes_moved / med / 1e6, 3)}


def measure(shapes, reps, warmup):
    numels = [_numel(s) for s in shapes]
    total = sum(numels)
    g = torch.Generator(device=DEV).manual_seed(7)
    resid = torch.randn(total, generator=g, device=DEV)
    views, o = [], 0
    for n in numels:
        views.append(resid[o:o + n])
        o += n
    ptrs = _lib.ptr_array([v.data_ptr() for v in views])
    b32 = torch.randn(total, generator=g, device=DEV) * 1e-3
    b16 = b32.bfloat16()
    g32, g16 = torch.empty_like(b32), torch.empty_like(b16)  # the gathers' own destinations
    same, ws_a = _table(numels, _lib.PSGD_F32, None)
    mixed, ws_b = _table(numels, _lib.PSGD_F32, _lib.PSGD_BF16)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    passes = {
        "add_f32": lambda: same.add(b32.data_ptr(), ptrs, stream),
        "add_mixed": lambda: mixed.add(b16.data_ptr(), ptrs, stream),
        "gather_f32": lambda: same.gather(g32.data_ptr(), ptrs, stream),
        "gather_mixed": lambda: mixed.gather(g16.data_ptr(), ptrs, stream),
    }
    for _ in range(warmup):
        for fn in passes.values():
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in passes}
    for _ in range(reps):  # alternating: every pass sees the same neighbours and machine state
        for k, fn in passes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {"elements": total, "runs": len(numels)}
    for k, evs in events.items():
        out[k] = _summary([a.elapsed_time(b) * 1e3 for a, b in evs], BYTES[k] * total)
    for op in ("add", "gather"):
        f, m = out[op + "_f32"], out[op + "_mixed"]
        out[op + "_ratio_mixed_over_f32"] = round(m["median_us"] / f["median_us"], 4)
        out[op + "_bar"] = round(1.0 + max(0.05, f["rel_spread"]), 4)  # 5 %, or the fp32 pass's own spread
    del ws_a, ws_b
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 50:
        raise SystemExit("--reps must be at least 50")
    if not torch.cuda.is_available():
        raise SystemExit("tools/runs_time.py needs a GPU")
    torch.cuda.set_device(DEV)
    res = {"tool": "runs_time", "device": torch.cuda.get_device_name(DEV), "reps": a.reps, "warmup": a.warmup,
           "workloads": {name: measure(shapes, a.reps, a.warmup) for name, shapes in WORKLOADS.items()}}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
