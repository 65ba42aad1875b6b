"""psgd_clip_outputs at world size W > 1.

W = 3 on one GPU through the stand-in collective library of tests/test_gpu_rccl_stub.py (its SUM
all-reduce writes W x the buffer: W ranks holding identical gradients): the factor form reads the
all-reduced factors with alpha = 1 / W and must agree with the stream form and with the norm of
the oracle workers' averaged outputs (oracle/multiworker.py), ranks 1 and 4 at I = 2, within the
per-step tolerance 1e-5 * ||input||.

W = 2 real processes on one GPU over the IPC exchange (PSGD_COMM=ipc): both ranks clip the same
averages and must report bit-identical norms and coefficients (every rank sums the factors in
rank order, and the norm's own sums have a fixed order)."""
import math
import os
import tempfile

import pytest
import torch

from test_gpu_rccl_stub import STUB, _init  # the stand-in collective library and its rendezvous

pytestmark = pytest.mark.gpu

SHAPES = [(64, 32, 3, 3), (64, 32, 3, 3), (64, 32, 3, 3), (3, 200), (96, 201), (256, 64, 1, 1), (40,), (130,)]
SCALES = [1.0, 4.0, 7.0, 1.0, 1.0, 1.0, 1.0, 1.0]
INF = float("inf")


def _mcr(rank, iters):
    """A min_compression_rate between the 1-D tensors' rates and the matrices' (reference
    powersgd.py:101-105, on the original shapes): every matrix compressed, the 1-D tensors not."""
    rate = lambda s: math.prod(s) / (0.5 * iters * min(rank, min(s)) * sum(s))  # noqa: E731
    lo, hi = max(rate(s) for s in SHAPES if len(s) == 1), min(rate(s) for s in SHAPES if len(s) > 1)
    assert lo < hi
    return math.sqrt(lo * hi)


def _norm64(tensors):
    return math.sqrt(sum(float((t.double().cpu() ** 2).sum()) for t in tensors))


def _stub_world3(_, init, rank, iters):
    os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
    os.environ["PSGD_TESTING"] = "1"
    os.environ["PSGD_STUB_MODE"] = "sum"
    from oracle import multiworker as MW
    from oracle import powersgd_oracle as O
    from powersgd_amd import Config, PowerSGD, _lib

    world = 3
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
    try:
        mcr = _mcr(rank, iters)
        psgd = PowerSGD([torch.zeros(s, device=dev) for s in SHAPES], Config(rank, mcr, iters, 0))
        assert psgd.is_compressed_mask == [True] * 6 + [False] * 2
        codec = psgd._powersgd
        codec._comm = _lib.Comm(world, 0, _lib.comm_unique_id(), 0)  # the stand-in, at world W
        states = []
        for _w in range(world):
            st = O.policy_init([torch.zeros(s) for s in SHAPES], rank, mcr, iters, 0)
            st.codec.p_flat.copy_(codec._ps_buffer.cpu())
            st.codec.q_flat.copy_(codec._qs_buffer.cpu())
            states.append(st)
        gen = torch.Generator().manual_seed(900 + rank)
        res_c = [[torch.zeros(s) for s in SHAPES] for _w in range(world)]
        res_d = [torch.zeros(s, device=dev) for s in SHAPES]
        stream = torch.cuda.current_stream().cuda_stream
        for step in range(2):
            new = [torch.randn(s, generator=gen) * k for s, k in zip(SHAPES, SCALES)]
            gd = [r + x.to(dev) for r, x in zip(res_d, new)]
            gc = [[r + x for r, x in zip(res_c[w], new)] for w in range(world)]
            scale = _norm64(gc[0])
            outs = psgd.aggregate(gd)
            torch.cuda.synchronize()
            assert codec._plan.norm_form(step, world) == _lib.Plan.NORM_FACTORS
            assert codec._plan.norm_form(step, 1) == _lib.Plan.NORM_STREAM  # recorded at world W
            got = {}
            for form in (_lib.Plan.NORM_FACTORS, _lib.Plan.NORM_STREAM):
                r = torch.zeros(2, dtype=torch.float64, device=dev)
                codec._plan.clip_outputs(step, world, codec._slab.data_ptr(), psgd._unc.slab.data_ptr(), psgd._unc.numel,
                                         INF, r.data_ptr(), stream, form)
                torch.cuda.synchronize()
                got[form] = float(r[0])
            want = MW.run_workers(states, gc)
            oracle = _norm64(want[0])
            fac, stm = got[_lib.Plan.NORM_FACTORS], got[_lib.Plan.NORM_STREAM]
            print(f"W=3 rank={rank} I={iters} step={step}: |factors - stream| / ||input|| = {abs(fac - stm) / scale:.3e}, "
                  f"|factors - oracle| / ||input|| = {abs(fac - oracle) / scale:.3e}")
            assert abs(stm - _norm64(outs)) <= 1e-10 * stm
            assert abs(fac - stm) <= 1e-5 * scale, (rank, step, fac, stm)
            assert abs(fac - oracle) <= 1e-5 * scale, (rank, step, fac, oracle)
            res_d, res_c = gd, gc
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("rank", [1, 4])
def test_factor_form_world3_vs_stream_and_oracle(rank, tmp_path):
    torch.multiprocessing.spawn(_stub_world3, args=(_init(tmp_path), rank, 2), nprocs=1, join=True)


def _ipc_worker(rank_id, world, initfile):
    os.environ["PSGD_COMM"] = "ipc"
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=world)
    try:
        from powersgd_amd import Config, PowerSGD, _lib

        dev = torch.device("cuda:0")
        psgd = PowerSGD([torch.zeros(s, device=dev) for s in SHAPES], Config(4, _mcr(4, 2), 2, 0))
        psgd.max_grad_norm = INF
        gen = torch.Generator().manual_seed(50 + rank_id)  # every rank its own gradients
        for step in range(2):
            grads = [(torch.randn(s, generator=gen) * k).to(dev) for s, k in zip(SHAPES, SCALES)]
            scales = [None] * world
            torch.distributed.all_gather_object(scales, _norm64(grads))
            outs = psgd.aggregate(grads)
            torch.cuda.synchronize()
            assert psgd._powersgd._plan.norm_form(step, world) == _lib.Plan.NORM_FACTORS
            norm = float(psgd.last_grad_norm)
            # the returned (on step 1: clipped) averages against the reported norm x coefficient
            assert abs(norm * float(psgd.last_clip_coef) - _norm64(outs)) <= 1e-5 * max(scales)
            psgd.max_grad_norm = norm / 2  # the next step clips
            mine = torch.stack([psgd.last_grad_norm, psgd.last_clip_coef]).cpu().view(torch.int64)
            both = [None] * world
            torch.distributed.all_gather_object(both, mine.tolist())
            assert both[0] == both[1], both  # bit-identical norm and coefficient on both ranks
            if step == 1:
                assert float(psgd.last_clip_coef) < 1.0
        assert not psgd._powersgd.ipc_status()
        psgd.close()
    finally:
        torch.distributed.destroy_process_group()


def test_ipc_two_ranks_report_identical_norm_and_coef():
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_ipc_worker, args=(2, os.path.join(td, "init")), nprocs=2, join=True)
