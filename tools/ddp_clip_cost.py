"""Cost of global-norm clipping in the default (fp32) DDP hook's one-call completion
(``direct_store = True``): the library's own clip (``PowerSGDState(..., max_grad_norm=x)``:
psgd_clip_dst after psgd_aggregate_comm_dst, the norm from the low-rank factors, the averages scaled
inside the buckets only when the norm exceeds x) against ``torch.nn.utils.clip_grad_norm_`` on the
parameters after the completion, interleaved in one process on ONE GPU.

Four states complete the same iteration, in an order that rotates every step:
  a  direct_store, no clipping (the code path without the keyword)
  b  direct_store, max_grad_norm = 1e30: a threshold nothing reaches (norm, finish, a scale launch
     whose workgroups return at once)
  c  direct_store, max_grad_norm = 1e-3: a threshold every step exceeds (every average re-read and
     scaled in the buckets)
  d  direct_store, no max_grad_norm, then torch.nn.utils.clip_grad_norm_(params, 1e30) with each
     p.grad the parameter's view of its bucket (what DDP leaves after backward)
What is timed: ``PowerSGDState._complete`` (d: and the torch call), from the arrival of the last
bucket (after its ADD) to the futures being set, between two stream events; per step, milliseconds.
Buckets and placements as tools/ddp_direct_cost.py (``aligned``: every view starts where the
previous one ends; ``offset``: one element in, every view 4-byte aligned only); ``cold``: a 1 GiB
buffer is rewritten before every step; ``warm``: steps back to back.

usage: python tools/ddp_clip_cost.py --ranks 1,4 --iters 2 --comm comm1|stub8 [--steps 40] [--warmup 8]
  comm1   a 1-rank communicator of the real collective library
  stub8   world 8 through the tests' stand-in collective library (PSGD_RCCL_LIB_FORCE)
Prints one JSON line per rank: per placement and mode the median / p10 / p90 of every form and the
medians' differences b - a, c - a, d - a in microseconds."""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
NEVER, ALWAYS = 1e30, 1e-3
FORMS = {"a_unclipped": None, "b_below": NEVER, "c_clips": ALWAYS, "d_torch": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="1,4")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--comm", choices=("stub8", "comm1"), required=True)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    if a.comm == "stub8":
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"
    import torch

    from powersgd_amd.workloads import resnet50_shapes

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    store = tempfile.mkdtemp()
    torch.distributed.init_process_group("gloo", init_method=f"file://{store}/init", rank=0, world_size=1)
    world = 8 if a.comm == "stub8" else 1
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float32, device=dev)) for s in resnet50_shapes()]
    flush = torch.zeros(1 << 28, dtype=torch.float32, device=dev)  # 1 GiB
    try:
        for rank in [int(r) for r in a.ranks.split(",")]:
            print(json.dumps(measure(a, rank, world, params, flush, dev)), flush=True)
    finally:
        torch.distributed.destroy_process_group()


def measure(a, rank, world, params, flush, dev):
    import torch
    from ddp_direct_cost import make_buckets

    from powersgd_amd import Config, _lib
    from powersgd_amd.ddp import PowerSGDState

    cfg = Config(rank, 2, a.iters, 0)
    res = {"tool": "ddp_clip_cost", "workload": "resnet50_fp32", "tensors": len(params), "rank": rank, "iters": a.iters,
           "comm": a.comm, "world": world, "steps": a.steps, "warmup": a.warmup,
           "unit": "ms per completion (last bucket's arrival to futures set; d: to the end of torch's clip), "
                   "stream events; deltas in us"}
    for placement, first in (("aligned", 0), ("offset", 1)):
        buckets = make_buckets(params, first, dev)
        view_of = {id(p): g for b in buckets for p, g in zip(b.parameters(), b.gradients())}
        states = {}
        for name, x in FORMS.items():
            st = PowerSGDState(cfg, params, max_grad_norm=x)
            st.direct_store = True
            st.powersgd._powersgd._comm = _lib.Comm(world, 0, _lib.comm_unique_id(), 0)
            st._events = []

            def timed(st=st, orig=st._complete, torch_clip=name == "d_torch"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                orig()
                if torch_clip:
                    torch.nn.utils.clip_grad_norm_(params, NEVER)
                e1.record()
                st._events.append((e0, e1))
            st._complete = timed
            states[name] = st
        res[f"{placement}_direct_store_applies"] = all(st.direct_store_applies() for st in states.values())
        for p in params:  # what DDP leaves in p.grad: the parameter's view of its bucket
            p.grad = view_of[id(p)]

        def step(st, cold):
            for b in buckets:
                b.buf.copy_(b.src)
            if cold:
                flush.add_(1.0)
            futs = [st._arrive(b) for b in buckets]
            assert all(f.done() for f in futs)

        names = list(states)
        for mode, cold in (("warm", False), ("cold", True)):
            for st in states.values():
                st._events.clear()
            for t in range(a.warmup + a.steps):
                k = t % len(names)
                for name in names[k:] + names[:k]:  # rotate the order
                    step(states[name], cold)
            torch.cuda.synchronize()
            med = {}
            for name, st in states.items():
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in st._events[a.warmup:])
                med[name] = statistics.median(ms)
                res[f"{placement}_{mode}_{name}"] = {"median": round(med[name], 4), "p10": round(ms[len(ms) // 10], 4),
                                                     "p90": round(ms[(len(ms) * 9) // 10], 4), "n": len(ms)}
            res[f"{placement}_{mode}_delta_us"] = {n: round(1e3 * (med[n] - med["a_unclipped"]), 1) for n in names[1:]}
        torch.cuda.synchronize()
        res[f"{placement}_coef"] = {n: float(states[n].last_clip_coef) for n in ("b_below", "c_clips")}
        res[f"{placement}_norms_equal"] = bool(torch.equal(states["b_below"].last_grad_norm.view(torch.int64),
                                                           states["c_clips"].last_grad_norm.view(torch.int64)))
        for p in params:
            p.grad = None
        for st in states.values():
            st.powersgd.close()
    return res


if __name__ == "__main__":
    main()
