"""tests/test_gpu_capped_rank.py's shape set (matrices whose own rank lies below the plan's rank
bucket) at world size 2, ranks 16, 32 and 64 with two iterations per step, fp32:

* psgd_aggregate_comm through the stand-in collective library (tests/stubs/rccl_stub.hip, the
  harness of tests/test_gpu_rccl_stub.py): one process, the communicator reports world 2 and its
  SUM all-reduce doubles the buffer, the SUM over two ranks holding identical gradients;
* the IPC exchange (PSGD_COMM=ipc, psgd_ipc_create at ranks 16 / 32, psgd_ipc_create2 at rank 64)
  with two processes on cuda:0 and distinct per-rank gradients.

Both against two reference workers (oracle/multiworker.py), every step from an identical state
(the oracle's P / Q are re-synchronised from the GPU object after every step), at TOL_STEP = 1e-5
of the larger input norm per tensor. The output slab is filled with NaN before every step and must
be finite after it. The skip table (tests/test_gpu_capped_rank.py: fp32 against float64 oracle
workers on the CPU) is empty for these cases."""
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
WORLD, ITERS = 2, 2


def _steps(kind, rank, rank_id, psgd):
    """STEPS steps of `psgd` (this process is worker `rank_id`) against WORLD oracle workers."""
    import test_gpu_capped_rank as C
    from oracle import multiworker as MW

    codec = psgd._powersgd
    states = [C.oracle_state(rank, ITERS) for _ in range(WORLD)]
    assert psgd.is_compressed_mask == states[0].mask
    C.check_plan(codec, rank)
    C.load_state(codec, states[0])
    for t in range(C.STEPS):
        for st in states:
            C.sync_state(st, codec)
        # the stand-in sums one rank's buffer WORLD times: identical gradients on every worker
        gc = [C.inputs(rank, ITERS, t, w if kind == "w2ipc" else 0) for w in range(WORLD)]
        scale = [max((gc[w][i] for w in range(WORLD)), key=lambda v: float(v.norm())).clone()
                 for i in range(len(C.SHAPES))]
        gd = C.to_device(gc[rank_id], torch.float32)
        ptr = C.poison(codec._slab)
        od = psgd.aggregate(gd)
        torch.cuda.synchronize()
        assert od[0].data_ptr() == ptr, "the step wrote another buffer than the one filled with NaN"
        found = C.Findings()
        found.expect(C.all_finite(codec._slab), kind, rank, t, "output slab not fully written")
        out = [o.cpu() for o in od]
        del od
        want = MW.run_workers(states, gc)
        for i, g in enumerate(scale):
            ctx = (kind, rank, ITERS, rank_id, t, i, C.SHAPES[i])
            found.expect(bool(torch.isfinite(out[i]).all()), *ctx, "output not fully written")
            found.expect(bool(torch.isfinite(gd[i]).all()), *ctx, "residual not finite")
            eo, er = C.rel(out[i], want[rank_id][i], g), C.rel(gd[i], gc[rank_id][i], g)
            print(f"{kind} rank {rank} worker {rank_id} step {t} tensor {i}: out {eo:.3e} res {er:.3e}")
            if (rank, ITERS, t, i) not in C.SKIP[kind]:
                found.check(eo, C.TOL_STEP, *ctx, "out")
                found.check(er, C.TOL_STEP, *ctx, "res")
        found.done()


def _stub_child(_, init, rank):
    os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
    os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
    os.environ["PSGD_STUB_MODE"] = "sum"
    import test_gpu_capped_rank as C
    from powersgd_amd import Config, PowerSGD, _lib

    torch.cuda.set_device(C.DEV)
    torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
    try:
        psgd = PowerSGD([torch.zeros(s, device=C.DEV) for s in C.SHAPES], Config(rank, C.MCR, ITERS, 0))
        # the library's own communicator, created through the stand-in at world 2 (the process
        # group itself has one rank: it only makes is_distributed() true)
        psgd._powersgd._comm = _lib.Comm(WORLD, 0, _lib.comm_unique_id(), 0)
        _steps("w2stub", rank, 0, psgd)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("rank", [16, 32, 64])
def test_stand_in_communicator_world2_vs_oracle(rank, tmp_path):
    torch.multiprocessing.spawn(_stub_child, args=(f"file://{tmp_path}/store", rank), nprocs=1, join=True)


def _ipc_worker(rank_id, initfile, rank):
    os.environ["PSGD_COMM"] = "ipc"
    os.environ.pop("PSGD_IPC_TWO_SHOT", None)  # auto
    import test_gpu_capped_rank as C
    from powersgd_amd import Config, PowerSGD

    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=WORLD)
    try:
        psgd = PowerSGD([torch.zeros(s, device=C.DEV) for s in C.SHAPES], Config(rank, C.MCR, ITERS, 0))
        _steps("w2ipc", rank, rank_id, psgd)
        assert psgd._powersgd._ipc_open
        assert not psgd._powersgd.ipc_status(), "a device-side exchange wait timed out"
        psgd.close()
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("rank", [16, 32, 64])
def test_ipc_exchange_two_processes_vs_oracle(rank):
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_ipc_worker, args=(os.path.join(td, "init"), rank), nprocs=WORLD, join=True)
