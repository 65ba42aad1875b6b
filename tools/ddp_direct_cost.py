"""Cost of the default (fp32) DDP hook's completion: ``direct_store = True``
(psgd_aggregate_comm_dst: one library call, the fp32 averages stored by the codec's final pass into
the buckets' gradient views) against the three-stage completion (psgd_aggregate_comm into an fp32
slab, then one run-table GATHER per bucket), interleaved A/B in one process on ONE GPU.

What is timed: ``PowerSGDState._complete``, from the arrival of the last bucket (after its ADD) to
the futures being set, between two stream events; per step, milliseconds. The buckets are the
hook's own interface driven directly (objects with GradBucket's methods: ~25 MB fp32 buffers, the
parameters back to back in reverse order, as DDP lays them out), so that the placement of the
gradient views is controlled:
  aligned   every view starts where the previous one ends
  offset    every bucket's views start one element in (every view 4-byte aligned only)
``cold``: a 1 GiB buffer is rewritten before every step (nothing of the step's data in the caches);
``warm``: steps back to back. Both states see the same gradients every step; their residuals and
P/Q are compared bit for bit at the end.

usage: python tools/ddp_direct_cost.py --ranks 1,2,4,16 --iters 2 --comm stub8|comm1 [--steps 40] [--warmup 8]
  stub8   world 8 through the tests' stand-in collective library (PSGD_RCCL_LIB_FORCE)
  comm1   a 1-rank communicator of the real collective library
  --parent  the library named by PSGD_LIB_PATH predates the one-call form: time the three stages only
Prints one JSON line per rank."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
BUCKET_ELEMS = 25 * (1 << 20) // 4  # DDP's default bucket_cap_mb of fp32 elements


class Bucket:
    """What ``powersgd_hook`` reads of a ``dist.GradBucket``."""

    def __init__(self, index, last, params, first, dev, gen):
        import torch

        numel = sum(p.numel() for p in params)
        self._index, self._last, self._params = index, last, params
        self.buf = torch.zeros(first + numel + 8, dtype=torch.float32, device=dev)
        self.src = torch.randn(self.buf.numel(), generator=gen, device=dev)
        self._grads, off = [], first
        for p in params:
            self._grads.append(self.buf[off:off + p.numel()].view(p.shape))
            off += p.numel()

    def index(self):
        return self._index

    def is_last(self):
        return self._last

    def parameters(self):
        return self._params

    def gradients(self):
        return self._grads

    def buffer(self):
        return self.buf


def make_buckets(params, first, dev):
    import torch

    gen = torch.Generator(device=dev).manual_seed(11)
    groups, cur, n = [], [], 0
    for p in reversed(params):
        cur.append(p)
        n += p.numel()
        if n >= BUCKET_ELEMS:
            groups.append(cur)
            cur, n = [], 0
    if cur:
        groups.append(cur)
    return [Bucket(i, i == len(groups) - 1, g, first, dev, gen) for i, g in enumerate(groups)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="1,2,4,16")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--comm", choices=("stub8", "comm1"), required=True)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--parent", action="store_true")
    a = ap.parse_args()
    if a.comm == "stub8":
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"
    import torch

    from powersgd_amd import Config, _lib
    from powersgd_amd.ddp import PowerSGDState
    from powersgd_amd.workloads import resnet50_shapes

    if a.parent:
        for name in ("psgd_aggregate_comm_dst", "psgd_aggregate_ipc_dst", "psgd_plan_dst_ok"):
            _lib._SIGNATURES.pop(name, None)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    import tempfile

    store = tempfile.mkdtemp()
    torch.distributed.init_process_group("gloo", init_method=f"file://{store}/init", rank=0, world_size=1)
    world = 8 if a.comm == "stub8" else 1
    shapes = resnet50_shapes()
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float32, device=dev)) for s in shapes]
    flush = torch.zeros(1 << 28, dtype=torch.float32, device=dev)  # 1 GiB
    try:
        for rank in [int(r) for r in a.ranks.split(",")]:
            print(json.dumps(measure(a, rank, world, params, flush, dev)), flush=True)
    finally:
        torch.distributed.destroy_process_group()


def measure(a, rank, world, params, flush, dev):
    import torch

    from powersgd_amd import Config, _lib
    from powersgd_amd.ddp import PowerSGDState

    cfg = Config(rank, 2, a.iters, 0)
    res = {"tool": "ddp_direct_cost", "workload": "resnet50_fp32", "rank": rank, "iters": a.iters, "comm": a.comm,
           "world": world, "steps": a.steps, "warmup": a.warmup,
           "library": os.path.basename(os.environ.get("PSGD_LIB_PATH", "in-tree")),
           "unit": "ms per completion (last bucket's arrival to futures set), stream events"}
    for placement, first in (("aligned", 0), ("offset", 1)):
        buckets = make_buckets(params, first, dev)
        ptrs = [g.data_ptr() for b in buckets for g in b.gradients()]
        res[f"{placement}_views"] = {"buckets": len(buckets), "align16": sum(p % 16 == 0 for p in ptrs),
                                     "align4_only": sum(p % 8 == 4 for p in ptrs)}
        states = {}
        for direct in ((False,) if a.parent else (True, False)):
            st = PowerSGDState(cfg, params)
            if direct:
                st.direct_store = True
            st.powersgd._powersgd._comm = _lib.Comm(world, 0, _lib.comm_unique_id(), 0)
            st._events = []

            def timed(st=st, orig=st._complete):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                orig()
                e1.record()
                st._events.append((e0, e1))
            st._complete = timed
            states["direct" if direct else "three_stage"] = st
        if not a.parent:
            res[f"{placement}_direct_store_applies"] = states["direct"].direct_store_applies()

        def step(st, cold):
            for b in buckets:
                b.buf.copy_(b.src)
            if cold:
                flush.add_(1.0)
            futs = [st._arrive(b) for b in buckets]
            assert all(f.done() for f in futs)

        for mode, cold in (("warm", False), ("cold", True)):
            for st in states.values():
                st._events.clear()
            names = list(states)
            for t in range(a.warmup + a.steps):
                for name in (names if t % 2 == 0 else names[::-1]):  # alternate the order
                    step(states[name], cold)
            torch.cuda.synchronize()
            for name, st in states.items():
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in st._events[a.warmup:])
                res[f"{placement}_{mode}_{name}"] = {"median": round(statistics.median(ms), 4),
                                                     "p10": round(ms[len(ms) // 10], 4),
                                                     "p90": round(ms[(len(ms) * 9) // 10], 4), "n": len(ms)}
        if not a.parent:
            f, u = states["direct"], states["three_stage"]
            res[f"{placement}_bitwise_equal"] = bool(
                torch.equal(f.residual.view(torch.int32), u.residual.view(torch.int32))
                and torch.equal(f.powersgd._powersgd._ps_buffer, u.powersgd._powersgd._ps_buffer)
                and torch.equal(f.powersgd._powersgd._qs_buffer, u.powersgd._powersgd._qs_buffer))
        for st in states.values():
            st.powersgd.close()
    return res


if __name__ == "__main__":
    main()
