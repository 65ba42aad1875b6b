"""The wide-rank path (effective ranks 33-128) at world size > 1.

* W = 2 gloo processes on one GPU with distinct per-rank gradients: the torch.distributed path
  (psgd_compress / all_reduce / psgd_decompress, ONE collective per iteration: wide plans take no
  buckets) against the oracle run in the same processes over the same group.
* psgd_aggregate_comm at W = 4 through the stand-in collective library (tests/stubs/
  rccl_stub.hip): the flat pack of the uncompressed 1-D tensor runs as its own launch, the step
  issues one collective per power iteration (the last one grouped with the flat tail), and the
  result matches W reference workers (oracle/multiworker.py).

Tolerances as in test_gpu_wide_rank.py: 1e-5 at step 0, 1e-4 at step 1."""
import ctypes
import os
import tempfile

import pytest
import torch

from parity_log import check

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")

SHAPES_A = [(300, 200), (200, 1000), (1000, 196), (256, 24, 3, 3), (197, 203), (300, 200), (40,)]
SHAPES_B = [(320, 300), (289, 1000), (1000, 288), (288, 32, 3, 3), (291, 293), (320, 300), (40,)]
SETS = {"A": SHAPES_A, "B": SHAPES_B}


def _rel(a, b, scale):
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(float(scale.double().norm()), 1e-30)


def _worker(rank_id, world, initfile, name, rank, iters, steps):
    from oracle import powersgd_oracle as O
    from powersgd_amd import Config, PowerSGD
    from powersgd_amd.workloads import hash_tensors

    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=world)
    try:
        shapes = SETS[name]
        dev = torch.device("cuda:0")
        psgd = PowerSGD([torch.zeros(s, device=dev) for s in shapes], Config(rank, 0.1, iters, 0))
        assert psgd._powersgd._plan.is_wide()
        ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 0.1, iters, 0)
        ora.codec.p_flat.copy_(psgd._powersgd._ps_buffer.cpu())
        ora.codec.q_flat.copy_(psgd._powersgd._qs_buffer.cpu())
        res_d = [torch.zeros(s, device=dev) for s in shapes]
        res_c = [torch.zeros(s) for s in shapes]
        for t in range(steps):
            new = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=900 + 10 * t + rank_id)]
            gd = [r + x.to(dev) for r, x in zip(res_d, new)]
            gc = [r + x for r, x in zip(res_c, new)]
            scale = [g.clone() for g in gc]
            od = psgd.aggregate(gd)
            oc = O.policy_step(ora, gc, world, lambda b: torch.distributed.all_reduce(b))
            torch.cuda.synchronize()
            for i, g in enumerate(scale):
                tol = 1e-5 if t == 0 else 1e-4
                check(_rel(od[i], oc[i], g), tol, name, rank, rank_id, t, i, "out")
                check(_rel(gd[i], gc[i], g), tol, name, rank, rank_id, t, i, "res")
            res_d, res_c = gd, gc
        assert len(psgd._powersgd._buckets) == 1
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("name,rank", [("A", 64), ("B", 128)])
def test_two_workers_vs_oracle(name, rank):
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_worker, args=(2, os.path.join(td, "init"), name, rank, 2, 2), nprocs=2, join=True)


def _comm_child(_, init, world, rank, iters, steps):
    os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
    os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
    os.environ["PSGD_STUB_MODE"] = "sum"
    from oracle import multiworker as MW
    from oracle import powersgd_oracle as O
    from powersgd_amd import Config, PowerSGD, _lib
    from powersgd_amd.workloads import hash_tensors

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
    try:
        stub = ctypes.CDLL(STUB)  # the same handle the library opened: one call counter
        stub.psgd_stub_calls.restype = ctypes.c_longlong
        shapes = SHAPES_A
        psgd = PowerSGD([torch.zeros(s, device=dev) for s in shapes], Config(rank, 0.1, iters, 0))
        codec = psgd._powersgd
        assert codec._plan.is_wide()
        nflat = sum(1 for m in psgd.is_compressed_mask if not m)
        assert nflat == 1  # the 1-D tensor is the flat tail
        codec._comm = _lib.Comm(world, 0, _lib.comm_unique_id(), 0)
        states = []
        for _w in range(world):
            st = O.policy_init([torch.zeros(s) for s in shapes], rank, 0.1, iters, 0)
            st.codec.p_flat.copy_(codec._ps_buffer.cpu())
            st.codec.q_flat.copy_(codec._qs_buffer.cpu())
            states.append(st)
        res_d = [torch.zeros(s, device=dev) for s in shapes]
        res_c = [[torch.zeros(s) for s in shapes] for _w in range(world)]
        for t in range(steps):
            new = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=700 + t)]
            gd = [r + x.to(dev) for r, x in zip(res_d, new)]
            gc = [[r + x for r, x in zip(res_c[w], new)] for w in range(world)]
            scale = [g.clone() for g in gc[0]]
            n0 = stub.psgd_stub_calls()
            od = psgd.aggregate(gd)
            torch.cuda.synchronize()
            calls = stub.psgd_stub_calls() - n0
            want = MW.run_workers(states, gc)
            tol = 1e-5 if t == 0 else 1e-4
            for i in range(len(shapes)):
                check(_rel(od[i], want[0][i], scale[i]), tol, "comm", world, t, i, "out")
                check(_rel(gd[i], gc[0][i], scale[i]), tol, "comm", world, t, i, "res")
            # one collective per power iteration; the last is a group of two all-reduce calls
            # (the factor and the flat tail), which the stand-in counts separately
            assert calls - nflat == iters, (calls, iters)
            res_d, res_c = gd, gc
    finally:
        torch.distributed.destroy_process_group()


def test_aggregate_comm_world4_vs_oracle(tmp_path):
    torch.multiprocessing.spawn(_comm_child, args=(f"file://{tmp_path}/store", 4, 64, 2, 2), nprocs=1, join=True)
