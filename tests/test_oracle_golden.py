"""Pin the CPU oracle against the reference's own outputs (golden fixtures).

The oracle (oracle/powersgd_oracle.py) must be BIT-IDENTICAL to the reference:
every comparison here is exact equality.
"""
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import powersgd_oracle as O
from golden_io import checksums, config_grads, config_state0, load, manifest, scenario_inputs
from powersgd_amd.workloads import CONFIGS, hash_tensors

MAN = manifest()


def _run_oracle_scenario(meta, rank_id=0, world=1, allreduce=None):
    shapes = [tuple(s) for s in meta["shapes"]]
    dtype = torch.float64 if meta["dtype"] == "f64" else torch.float32
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        params = [torch.zeros(s, dtype=dtype) for s in shapes]
        ps = O.policy_init(params, meta["rank"], meta["mcr"], meta["iters"], meta["start"])
        rec = {"mask": np.array(ps.mask), "p0": ps.codec.p_flat.numpy().copy(),
               "q0": ps.codec.q_flat.numpy().copy(),
               "compression_rate": np.array(O.codec_compression_rate(ps.codec))}
        res = [torch.zeros(s, dtype=dtype) for s in shapes]
        for t in range(meta["steps"]):
            grads = scenario_inputs(meta, t, res, rank_id, dtype)
            outs = O.policy_step(ps, grads, world, allreduce)
            for i in range(len(shapes)):
                rec[f"s{t}_out_{i}"] = outs[i].numpy().copy()
                rec[f"s{t}_res_{i}"] = grads[i].numpy().copy()
            rec[f"s{t}_p"] = ps.codec.p_flat.numpy().copy()
            rec[f"s{t}_q"] = ps.codec.q_flat.numpy().copy()
            rec[f"s{t}_step"] = np.array([ps.step, ps.codec.step])
            res = grads
    finally:
        torch.set_default_dtype(prev)
    return rec


def _assert_same(got, want, prefix=""):
    assert set(want) <= set(got), sorted(set(want) - set(got))
    for k, v in want.items():
        g = got[k]
        assert g.shape == v.shape and g.dtype == v.dtype, (prefix + k, g.shape, v.shape, g.dtype, v.dtype)
        assert np.array_equal(g, v), f"{prefix}{k}: max|d|={np.max(np.abs(g - v))}"


@pytest.mark.parametrize("name", sorted(MAN["scenarios"]))
def test_oracle_bitwise_single_worker(name):
    meta = MAN["scenarios"][name]
    _assert_same(_run_oracle_scenario(meta), load("F1_" + name))


def _gloo_worker(rank_id, world, meta, initfile, outdir):
    torch.distributed.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank_id,
                                         world_size=world)
    torch.set_num_threads(1)
    rec = _run_oracle_scenario(meta, rank_id, world, lambda b: torch.distributed.all_reduce(b))
    np.savez(os.path.join(outdir, f"r{rank_id}.npz"), **rec)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("key", sorted(MAN["multi"]))
def test_oracle_bitwise_multi_worker_gloo(key):
    info = MAN["multi"][key]
    meta = dict(MAN["scenarios"][info["scenario"]])
    world = info["world"]
    want = load("F2_" + key)
    with tempfile.TemporaryDirectory() as td:
        torch.multiprocessing.spawn(_gloo_worker, args=(world, meta, os.path.join(td, "init"), td),
                                    nprocs=world, join=True)
        for r in range(world):
            with np.load(os.path.join(td, f"r{r}.npz")) as z:
                got = {f"rank{r}_{k}": z[k] for k in z.files}
            _assert_same(got, {k: v for k, v in want.items() if k.startswith(f"rank{r}_")})


@pytest.mark.parametrize("cfg", sorted(MAN["configs"]))
def test_oracle_config_checksums(cfg):
    info = MAN["configs"][cfg]
    c = CONFIGS[cfg]
    want = load(f"{info['tag']}_{cfg}")
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    params = [torch.zeros(s) for s in c["shapes"]]
    ps = O.policy_init(params, c["rank"], c["mcr"], c["iters"], 0)
    p0, q0 = config_state0(ps.codec.p_flat.numel(), ps.codec.q_flat.numel())
    ps.codec.p_flat.copy_(p0)
    ps.codec.q_flat.copy_(q0)
    assert np.array_equal(np.array(ps.mask), want["mask"])
    grads = [torch.zeros(s) for s in c["shapes"]]
    for t in range(info["steps"]):
        grads = config_grads(cfg, t, grads)
        outs = O.policy_step(ps, grads)
        for i in range(len(grads)):
            so, no, xo = checksums(outs[i].numpy())
            sr, nr, xr = checksums(grads[i].numpy())
            assert np.array_equal(np.array([so, no, sr, nr]), want[f"s{t}_sums"][i]), (cfg, t, i)
        assert ps.codec.p_flat.double().sum().item() == want[f"s{t}_p_sum"]
        assert ps.codec.q_flat.double().sum().item() == want[f"s{t}_q_sum"]


def test_oracle_matches_reference_random_shapes():
    """The reference's recorded steps on a mixed shape set (F5, tests/golden/make_golden_random.py:
    three (rank, iterations) cases, three steps each with error feedback): initial state, outputs
    and residuals, bitwise."""
    want = load("F5_random_shapes")
    shapes = [(40, 30), (40, 30), (7, 5, 2), (9,), (128, 3, 3), (5, 300)]
    seen = set()
    for ci, (rank, iters) in enumerate(((1, 2), (3, 3), (2, 1))):
        ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 1.5, iters, 0)
        got = {f"c{ci}_p0": ora.codec.p_flat.numpy().copy(), f"c{ci}_q0": ora.codec.q_flat.numpy().copy()}
        grads = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=3000 + 10 * ci)]
        for t in range(3):
            outs = O.policy_step(ora, grads)
            for i in range(len(shapes)):
                got[f"c{ci}_s{t}_out_{i}"] = outs[i].numpy().copy()
                got[f"c{ci}_s{t}_res_{i}"] = grads[i].numpy().copy()
            for g, f in zip(grads, hash_tensors(shapes, seed=3000 + 10 * ci + t + 1)):
                g.add_(torch.from_numpy(f))
        _assert_same(got, {k: v for k, v in want.items() if k.startswith(f"c{ci}_")}, "F5 ")
        seen |= set(got)
    assert seen == set(want)  # every recorded array was compared
