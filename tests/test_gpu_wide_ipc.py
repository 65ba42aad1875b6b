"""The IPC exchange (PSGD_COMM=ipc) for wide plans, effective ranks 33-128, and its two-shot form
(psgd_ipc_create2; k_xchg_rs + k_xchg_ag, psgd_xchg2.hip). W processes on cuda:0 over a gloo store.

a. against the oracle (policy_step with torch.distributed.all_reduce, distinct per-rank
   gradients), auto mode: the wide-rank tolerances, 1e-5 at step 0 and 1e-4 at step 1;
b. one-shot against two-shot, bit for bit, at ragged shard ends and a ragged flat tail, and the
   outputs bitwise equal across ranks;
c. the same under skewed arrival;
d. the old entry keeps refusing wide plans, and a narrow plan through psgd_ipc_create2 is
   psgd_ipc_create's session bit for bit."""
import os
import tempfile
import time

import pytest
import torch

from golden_io import load, manifest, scenario_inputs
from parity_log import check

pytestmark = pytest.mark.gpu

# the wide-rank shape sets of tests/test_gpu_wide_rank_multi.py
SHAPES_A = [(300, 200), (200, 1000), (1000, 196), (256, 24, 3, 3), (197, 203), (300, 200), (40,)]
SHAPES_B = [(320, 300), (289, 1000), (1000, 288), (288, 32, 3, 3), (291, 293), (320, 300), (40,)]
SETS = {"A": SHAPES_A, "B": SHAPES_B}

# (37, 50) has effective rank 37 and (200, 1) rank 1 (at minimum compression rate 0.1 it is
# compressed too): P total 300 * 64 + 37 * 37 + 200 = 20769 (= 1 mod 4), Q total 200 * 64 + 50 * 37
# + 1 = 14651 (= 3 mod 4), so the last quad of either factor is ragged and at W = 4 the last shard
# is shorter than the others; (41,) stays uncompressed: a flat tail of 10 quads + 1
# Set S: the same without the rank-1 matrix and with the flat tail it would otherwise have made
# (200 + 41 values, 60 quads + 1): P total 20569 (odd), Q total 14650 (= 2 mod 4)
RAGGED = {"R": ([(300, 200), (37, 50), (200, 1), (41,)], [True, True, True, False], (20769, 14651)),
          "S": ([(300, 200), (37, 50), (241,)], [True, True, False], (20569, 14650))}
SHAPES_R = RAGGED["R"][0]


def _rel(a, b, scale):
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(float(scale.double().norm()), 1e-30)


def _init(rank_id, world, initfile):
    os.environ["PSGD_COMM"] = "ipc"
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id, world_size=world)


# ------------------------------------------------------------------ a. against the oracle --
def _oracle_worker(rank_id, world, initfile, name, rank, iters, steps):
    from oracle import powersgd_oracle as O
    from powersgd_amd import Config, PowerSGD
    from powersgd_amd.workloads import hash_tensors

    os.environ.pop("PSGD_IPC_TWO_SHOT", None)  # auto
    _init(rank_id, world, initfile)
    try:
        shapes = SETS[name]
        dev = torch.device("cuda:0")
        psgd = PowerSGD([torch.zeros(s, device=dev) for s in shapes], Config(rank, 0.1, iters, 0))
        codec = psgd._powersgd
        assert codec._plan.is_wide()
        ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 0.1, iters, 0)
        ora.codec.p_flat.copy_(codec._ps_buffer.cpu())
        ora.codec.q_flat.copy_(codec._qs_buffer.cpu())
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
                check(_rel(od[i], oc[i], g), tol, "wide-ipc", name, rank, world, rank_id, t, i, "out")
                check(_rel(gd[i], gc[i], g), tol, "wide-ipc", name, rank, world, rank_id, t, i, "res")
            res_d, res_c = gd, gc
        assert codec._ipc_open
        # auto: two-shot where the world is >= 3 and the factor is >= 512 KiB
        pn, qn = codec._plan.factor_numel()
        for side, numel in ((0, pn), (1, qn)):
            assert codec._plan.ipc_two_shot(side) == (world >= 3 and 4 * numel >= 512 * 1024), (side, numel, world)
        assert not codec.ipc_status(), "a device-side exchange wait timed out"
        psgd.close()
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("name,rank,world", [("A", 64, 2), ("B", 128, 2), ("A", 64, 3)])
def test_wide_ipc_vs_oracle(name, rank, world):
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_oracle_worker, args=(world, os.path.join(td, "init"), name, rank, 2, 2),
                                    nprocs=world, join=True)


# ------------------------------------------- b / c. one-shot against two-shot, bit for bit --
def _run_ragged(rank_id, world, two_shot, skew, name="R"):
    """One codec over a RAGGED set (rank 64, I = 3, 3 steps) in the forced form; after every step the
    outputs, the residuals and the P / Q buffers (CPU copies). Collective: closes its session."""
    from powersgd_amd import Config, PowerSGD
    from powersgd_amd.workloads import hash_tensors

    os.environ["PSGD_IPC_TWO_SHOT"] = "1" if two_shot else "0"
    dev = torch.device("cuda:0")
    shapes, mask, totals = RAGGED[name]
    psgd = PowerSGD([torch.zeros(s, device=dev) for s in shapes], Config(64, 0.1, 3, 0))
    codec = psgd._powersgd
    assert codec._plan.is_wide() and [bool(m) for m in psgd.is_compressed_mask] == mask
    assert codec._plan.factor_numel() == totals
    res = [torch.zeros(s, device=dev) for s in shapes]
    snaps = []
    for t in range(3):
        new = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=300 + 10 * t + rank_id)]
        grads = [r + x.to(dev) for r, x in zip(res, new)]
        if skew and rank_id == t % world:
            time.sleep(0.3)  # this rank arrives late at every exchange of the step
        outs = psgd.aggregate(grads)
        torch.cuda.synchronize()
        snaps.append({"out": [o.cpu().clone() for o in outs], "res": [g.cpu().clone() for g in grads],
                      "P": codec._ps_buffer.cpu().clone(), "Q": codec._qs_buffer.cpu().clone()})
        res = grads
    # the session ran the form it was asked for, on both sides: else the comparison proves nothing
    assert codec._plan.ipc_two_shot(0) == two_shot and codec._plan.ipc_two_shot(1) == two_shot
    assert not codec.ipc_status(), "a device-side exchange wait timed out"
    psgd.close()
    return snaps


def _same_bits(a, b, what):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in ("out", "res"):
            for i, (u, v) in enumerate(zip(x[k], y[k])):
                assert torch.equal(u, v), (what, t, k, i)  # the outputs include the uncompressed averages
        assert torch.equal(x["P"], y["P"]) and torch.equal(x["Q"], y["Q"]), (what, t, "P/Q")


def _ragged_worker(rank_id, world, initfile, skew, name="R"):
    _init(rank_id, world, initfile)
    try:
        if skew:
            ref = _run_ragged(rank_id, world, True, False)
            got = _run_ragged(rank_id, world, True, True)
        else:
            ref = _run_ragged(rank_id, world, False, False, name)
            got = _run_ragged(rank_id, world, True, False, name)
        for s in got:
            assert all(bool(torch.isfinite(o).all()) for o in s["out"])
        _same_bits(ref, got, "skewed" if skew else "two-shot vs one-shot")
        # every rank sums in rank order: a mis-gathered shard on one rank shows up here
        mine = [s["out"] for s in got]
        every = [None] * world
        torch.distributed.all_gather_object(every, mine)
        for w, theirs in enumerate(every):
            for t in range(len(mine)):
                for i, (u, v) in enumerate(zip(mine[t], theirs[t])):
                    assert torch.equal(u, v), ("across ranks", rank_id, w, t, i)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world", [3, 4])
@pytest.mark.parametrize("name", sorted(RAGGED))
def test_two_shot_equals_one_shot_bitwise(name, world):
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_ragged_worker, args=(world, os.path.join(td, "init"), False, name),
                                    nprocs=world, join=True)


def test_two_shot_skewed_ranks():
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_ragged_worker, args=(3, os.path.join(td, "init"), True), nprocs=3, join=True)


# ------------------------------------------------------------------ d. old entry unchanged --
def test_old_entry_refuses_wide_plans():
    from powersgd_amd import Config, PowerSGD

    dev = torch.device("cuda:0")
    psgd = PowerSGD([torch.zeros(s, device=dev) for s in SHAPES_R], Config(64, 0.1, 2, 0))
    plan = psgd._powersgd._plan
    assert plan.is_wide()
    with pytest.raises(ValueError, match="psgd_ipc_create: ranks above 32 are not supported there"):
        plan.ipc_create(0)
    with pytest.raises(RuntimeError, match="STATE.*psgd_ipc_open first"):
        plan.ipc_two_shot(0)


def _narrow_session(rank_id, key, mode):
    """The F2 scenario of `key` over PSGD_COMM=ipc; mode None: the session of psgd_ipc_create,
    else of psgd_ipc_create2(mode)."""
    from powersgd_amd import Config, PowerSGD, _lib

    man = manifest()
    meta = man["scenarios"][man["multi"][key]["scenario"]]
    want = load("F2_" + key)
    pre = f"rank{rank_id}_"
    dev = torch.device("cuda:0")
    shapes = [tuple(s) for s in meta["shapes"]]
    psgd = PowerSGD([torch.zeros(s, device=dev) for s in shapes],
                    Config(meta["rank"], meta["mcr"], meta["iters"], meta["start"]))
    codec = psgd._powersgd
    assert not codec._plan.is_wide()
    codec._ps_buffer.copy_(torch.from_numpy(want[pre + "p0"]).to(dev))
    codec._qs_buffer.copy_(torch.from_numpy(want[pre + "q0"]).to(dev))
    old = _lib.Plan.ipc_create
    if mode is not None:
        _lib.Plan.ipc_create = lambda self, flat_numel=0: self.ipc_create2(flat_numel, mode)
    snaps = []
    try:
        res = [torch.zeros(s) for s in shapes]
        for t in range(meta["steps"]):
            grads = [g.to(dev) for g in scenario_inputs(meta, t, res, rank_id)]
            outs = psgd.aggregate(grads)
            torch.cuda.synchronize()
            snaps.append({"out": [o.cpu().clone() for o in outs], "res": [g.cpu().clone() for g in grads],
                          "P": codec._ps_buffer.cpu().clone(), "Q": codec._qs_buffer.cpu().clone()})
            res = [g.cpu() for g in grads]
        assert codec._ipc_open and not codec._plan.ipc_two_shot(0) and not codec._plan.ipc_two_shot(1)
        assert not codec.ipc_status()
        psgd.close()
    finally:
        _lib.Plan.ipc_create = old
    return snaps


def _narrow_worker(rank_id, initfile, key):
    from powersgd_amd import Config, PowerSGD

    _init(rank_id, 2, initfile)
    try:
        ref = _narrow_session(rank_id, key, None)
        for mode in (0, 2):
            _same_bits(ref, _narrow_session(rank_id, key, mode), f"create2 mode {mode}")
        # two-shot is not built for ranks up to 32
        dev = torch.device("cuda:0")
        plan = PowerSGD([torch.zeros(64, 32, device=dev)], Config(2, 1, 2, 0))._powersgd._plan
        with pytest.raises(ValueError, match="two-shot exchange serves ranks above 32"):
            plan.ipc_create2(0, 1)
    finally:
        torch.distributed.destroy_process_group()


def test_narrow_plan_through_create2_is_create():
    man = manifest()
    key = sorted(k for k in man["multi"] if man["multi"][k]["world"] == 2)[0]
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_narrow_worker, args=(os.path.join(td, "init"), key), nprocs=2, join=True)
