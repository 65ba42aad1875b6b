"""What the DDP hook's completion costs at ranks 64 and 128: the one-call forms on a wide plan
(psgd_aggregate_comm_dst_wide / psgd_aggregate_mixed_comm_dst_wide: the final pass k_wide_apply_dst stores
the averages into the buckets' gradient views) against the three-stage completion (psgd_aggregate_comm into
an fp32 slab, then one run-table GATHER per bucket), interleaved in one process on ONE GPU.

    python tools/ddp_wide_time.py [--steps 20] [--warmup 4] [--parent] [--out profiles/ddp_wide/ddp_wide_time.jsonl]

A one-rank gloo group and a 1-rank communicator of the collective library (the transport the wide entries
serve). Shapes: ResNet-50 (two iterations per step) and the Llama-7B layer shapes (one iteration), each at
ranks 64 and 128, in both forms: "f32" (fp32 buckets, ``direct_store = True`` against a plain state) and
"bf16" (bf16 buckets over an fp32 residual, ``fused=True`` against ``fused=False``). What is timed:
``PowerSGDState._complete``, from the arrival of the last bucket (after its ADD) to the futures being set,
between two stream events, as tools/ddp_direct_cost.py times it; the buckets are the hook's own interface
driven directly (~25 MB buffers, the parameters back to back in reverse order, as DDP lays them out). Both
states see the same gradients every step, in alternating order; their residuals and P / Q are compared bit
for bit at the end. Per state the median, p10 and p90 over the steps; a difference counts only beyond the
spread (p90 - p10) of both. One JSON line per row.
  --parent  the library named by PSGD_LIB_PATH predates the wide entries: time the three stages only"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from ddp_direct_cost import BUCKET_ELEMS, Bucket  # noqa: E402  (tools/: the hook's bucket interface)

NEW = ("psgd_aggregate_comm_dst_wide", "psgd_plan_dst_wide_ok", "psgd_aggregate_mixed_comm_dst_wide",
       "psgd_plan_mixed_dst_wide_ok")
ROWS = [(name, rank, form) for name in ("cfg3_resnet50_r4", "cfg4_llama_r2_bf16") for rank in (64, 128)
        for form in ("f32", "bf16")]


def make_buckets(params, dev):
    import torch

    gen = torch.Generator(device=dev).manual_seed(11)
    per = BUCKET_ELEMS * 4 // params[0].element_size()
    groups, cur, n = [], [], 0
    for p in reversed(params):
        cur.append(p)
        n += p.numel()
        if n >= per:
            groups.append(cur)
            cur, n = [], 0
    if cur:
        groups.append(cur)
    out = []
    for i, g in enumerate(groups):
        b = Bucket(i, i == len(groups) - 1, g, 0, dev, gen)
        if params[0].dtype != torch.float32:  # Bucket builds fp32 buffers: the same layout in the parameters' dtype
            b.buf, b.src = b.buf.to(params[0].dtype), b.src.to(params[0].dtype)
            off, b._grads = 0, []
            for p in g:
                b._grads.append(b.buf[off:off + p.numel()].view(p.shape))
                off += p.numel()
        out.append(b)
    return out


def measure(a, name, rank, form, dev):
    import torch

    from powersgd_amd import Config, _lib
    from powersgd_amd.ddp import PowerSGDState
    from powersgd_amd.workloads import CONFIGS

    c = CONFIGS[name]
    dt = torch.float32 if form == "f32" else torch.bfloat16
    params = [torch.nn.Parameter(torch.zeros(s, dtype=dt, device=dev)) for s in c["shapes"]]
    buckets = make_buckets(params, dev)
    cfg = Config(rank, c["mcr"], c["iters"], 0)
    res = {"tool": "ddp_wide_time", "shapes": name, "rank": rank, "iters": c["iters"], "form": form, "steps": a.steps,
           "warmup": a.warmup, "buckets": len(buckets), "library": os.path.basename(os.environ.get("PSGD_LIB_PATH", "in-tree")),
           "unit": "ms per completion (last bucket's arrival to futures set), stream events"}
    states = {}
    for one_call in ((False,) if a.parent else (True, False)):
        if form == "f32":
            st = PowerSGDState(cfg, params)
            st.direct_store = one_call
        else:
            st = PowerSGDState(cfg, params, residual_dtype=torch.float32, fused=one_call)
        st.powersgd._powersgd._comm = _lib.Comm(1, 0, _lib.comm_unique_id(), 0)
        st._events = []

        def timed(st=st, orig=st._complete):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            orig()
            e1.record()
            st._events.append((e0, e1))
        st._complete = timed
        states["one_call" if one_call else "three_stage"] = st
    if not a.parent:
        st = states["one_call"]
        res["one_call_applies"] = bool(st.direct_store_applies() if form == "f32" else st.fused_folds() == (0, 1))
    plan = st.powersgd._powersgd._plan
    res["wide"], res["compressed_elements"] = bool(plan.is_wide()), int(sum(
        p.numel() for p, m in zip(params, st.powersgd.is_compressed_mask) if m))
    names = list(states)
    for t in range(a.warmup + a.steps):
        for k in (names if t % 2 == 0 else names[::-1]):  # alternate the order
            for b in buckets:
                b.buf.copy_(b.src)
            assert all(f.done() for f in [states[k]._arrive(b) for b in buckets])
    torch.cuda.synchronize()
    for k, st in states.items():
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in st._events[a.warmup:])
        res[k] = {"median": round(statistics.median(ms), 4), "p10": round(ms[len(ms) // 10], 4),
                  "p90": round(ms[(len(ms) * 9) // 10], 4), "n": len(ms)}
    if not a.parent:
        f, u = states["one_call"], states["three_stage"]
        res["one_call_minus_three_stage_ms"] = round(res["one_call"]["median"] - res["three_stage"]["median"], 4)
        res["bitwise_equal"] = bool(
            torch.equal(f.residual.view(torch.int32), u.residual.view(torch.int32))
            and torch.equal(f.powersgd._powersgd._ps_buffer, u.powersgd._powersgd._ps_buffer)
            and torch.equal(f.powersgd._powersgd._qs_buffer, u.powersgd._powersgd._qs_buffer))
    for st in states.values():
        st.powersgd.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from powersgd_amd import _lib

    if a.parent:
        for name in NEW:
            _lib._SIGNATURES.pop(name, None)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.distributed.init_process_group("gloo", init_method=f"file://{tempfile.mkdtemp()}/init", rank=0, world_size=1)
    lines = []
    try:
        for name, rank, form in ROWS:
            lines.append(json.dumps(measure(a, name, rank, form, dev)))
            print(lines[-1], flush=True)
            if a.out:  # after every row: a run cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
            torch.cuda.empty_cache()
    finally:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
