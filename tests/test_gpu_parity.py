"""GPU parity: the HIP path (through libpsgd's C ABI) against the reference.

* golden fixtures (produced by the reference itself) — per step from the reference's
  own state/residual (tight), and free-running over several steps (looser: the warm
  start amplifies rounding differences);
* the CPU oracle (bit-identical to the reference) at every BASELINE config at full size;
* size-independent properties: error-feedback identity out + residual == input at
  world size 1, bitwise determinism, orthonormal factors.

Tolerances (fp32 floating point; north_star asks for a stated fp32 tolerance): per
tensor ||ours - ref||_F <= TOL * ||input||_F with TOL_STEP = 1e-5 per step from an
identical state (TOL_STEP_R1 = 1e-6 at rank 1) and TOL_FREE = 1e-4 for up to 4
free-running steps; bf16 gradients (reference cannot run them) compare against the oracle
on bf16-rounded inputs with TOL_BF16 = 4e-3. Every comparison's error is logged
(tests/parity_log.py); DESIGN.md §5 quotes the worst observed values.
"""
import os

import numpy as np
import pytest
import torch

from golden_io import checksums, config_grads, config_state0, load, manifest, scenario_inputs
from parity_log import check
from oracle import powersgd_oracle as O
from powersgd_amd import Config, PowerSGD
from powersgd_amd.workloads import CONFIGS, hash_tensors, resnet50_shapes

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-5
TOL_STEP_R1 = 1e-6  # rank 1: same op order as the reference up to summation order
TOL_FREE = 1e-4
TOL_BF16 = 4e-3
DEV = torch.device("cuda:0")
MAN = manifest()


def _rel(a: torch.Tensor, b: torch.Tensor, scale: torch.Tensor) -> float:
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(float(scale.double().norm()), 1e-30)


def _new_gpu(meta):
    shapes = [tuple(s) for s in meta["shapes"]]
    params = [torch.zeros(s, device=DEV) for s in shapes]
    return PowerSGD(params, Config(meta["rank"], meta["mcr"], meta["iters"], meta["start"]))


def _inject(psgd, p, q, steps):
    psgd._powersgd._ps_buffer.copy_(torch.from_numpy(np.ascontiguousarray(p)).to(DEV))
    psgd._powersgd._qs_buffer.copy_(torch.from_numpy(np.ascontiguousarray(q)).to(DEV))
    psgd.step_counter, psgd._powersgd.step_counter = int(steps[0]), int(steps[1])


F32_SCENARIOS = sorted(k for k, v in MAN["scenarios"].items() if v["dtype"] == "f32")


@pytest.mark.parametrize("name", F32_SCENARIOS)
def test_golden_per_step(name):
    """Each step starts from the reference's own state and residual."""
    meta = MAN["scenarios"][name]
    want = load("F1_" + name)
    shapes = [tuple(s) for s in meta["shapes"]]
    psgd = _new_gpu(meta)
    assert psgd.is_compressed_mask == list(want["mask"])
    tol = TOL_STEP_R1 if meta["rank"] == 1 else TOL_STEP
    res_ref = [torch.zeros(s) for s in shapes]
    for t in range(meta["steps"]):
        if t == 0:
            _inject(psgd, want["p0"], want["q0"], (0, 0))
        else:
            _inject(psgd, want[f"s{t-1}_p"], want[f"s{t-1}_q"], want[f"s{t-1}_step"])
        inputs = scenario_inputs(meta, t, res_ref)
        grads = [g.to(DEV) for g in inputs]
        outs = psgd.aggregate(grads)
        torch.cuda.synchronize()
        for i, g in enumerate(inputs):
            wo = torch.from_numpy(want[f"s{t}_out_{i}"])
            wr = torch.from_numpy(want[f"s{t}_res_{i}"])
            check(_rel(outs[i], wo, g), tol, name, t, i, "out")
            check(_rel(grads[i], wr, g), tol, name, t, i, "res")
        assert [psgd.step_counter, psgd._powersgd.step_counter] == list(want[f"s{t}_step"])
        res_ref = [torch.from_numpy(want[f"s{t}_res_{i}"]) for i in range(len(shapes))]


@pytest.mark.parametrize("name", F32_SCENARIOS)
def test_golden_free_running(name):
    meta = MAN["scenarios"][name]
    want = load("F1_" + name)
    shapes = [tuple(s) for s in meta["shapes"]]
    psgd = _new_gpu(meta)
    _inject(psgd, want["p0"], want["q0"], (0, 0))
    res = [torch.zeros(s) for s in shapes]
    for t in range(meta["steps"]):
        inputs = scenario_inputs(meta, t, res)
        grads = [g.to(DEV) for g in inputs]
        outs = psgd.aggregate(grads)
        torch.cuda.synchronize()
        for i, g in enumerate(inputs):
            wo = torch.from_numpy(want[f"s{t}_out_{i}"])
            wr = torch.from_numpy(want[f"s{t}_res_{i}"])
            check(_rel(outs[i], wo, g), TOL_FREE, name, t, i, "out")
            check(_rel(grads[i], wr, g), TOL_FREE, name, t, i, "res")
        res = [x.cpu() for x in grads]


def test_warmup_passthrough_like_reference_test():
    """Mirror of the reference's test_no_compression_in_the_beginning (tests/powersgd_test.py:14-34)."""
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 100, 3), torch.nn.ReLU(), torch.nn.Conv2d(100, 50, 5),
                                torch.nn.Linear(50, 1)).to(DEV)
    params = list(model.parameters())
    psgd = PowerSGD(params, Config(rank=1, min_compression_rate=10, start_compressing_after_num_steps=2,
                                   num_iters_per_step=1))
    grads = [torch.randn_like(p) for p in params]
    orig = [g.clone() for g in grads]
    avg = psgd.aggregate(grads)
    for g in grads:
        assert torch.equal(g, torch.zeros_like(g))
    for a, o in zip(avg, orig):
        assert torch.equal(a, o)
    assert psgd.step_counter == 1


def test_error_feedback_identity_like_reference_test():
    """Mirror of test_error_feedback_mechanism (tests/powersgd_test.py:37-55), fp32 on GPU."""
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 100, 3), torch.nn.ReLU(), torch.nn.Conv2d(100, 50, 5),
                                torch.nn.Linear(50, 1)).to(DEV)
    params = list(model.parameters())
    psgd = PowerSGD(params, Config(rank=2, min_compression_rate=10, start_compressing_after_num_steps=0,
                                   num_iters_per_step=3))
    grads = [torch.randn_like(p) for p in params]
    orig = [g.clone() for g in grads]
    avg = psgd.aggregate(grads)
    for o, a, b in zip(orig, avg, grads):
        assert torch.allclose(o, a + b, rtol=1e-5, atol=1e-6)


def _oracle_and_gpu(cfg, steps, dtype=torch.float32):
    c = CONFIGS[cfg]
    shapes = c["shapes"]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ps = O.policy_init([torch.zeros(s) for s in shapes], c["rank"], c["mcr"], c["iters"], 0)
    p0, q0 = config_state0(ps.codec.p_flat.numel(), ps.codec.q_flat.numel())
    ps.codec.p_flat.copy_(p0)
    ps.codec.q_flat.copy_(q0)
    gpu = PowerSGD([torch.zeros(s, device=DEV, dtype=dtype) for s in shapes],
                   Config(c["rank"], c["mcr"], c["iters"], 0))
    gpu._powersgd._ps_buffer.copy_(p0.to(DEV))
    gpu._powersgd._qs_buffer.copy_(q0.to(DEV))
    res_cpu = [torch.zeros(s) for s in shapes]
    res_gpu = [torch.zeros(s, device=DEV, dtype=dtype) for s in shapes]
    for t in range(steps):
        fresh = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=2000 + t)]
        g_gpu = [(r + f.to(DEV)).to(dtype) for r, f in zip(res_gpu, fresh)]
        g_cpu = [g.float().cpu() for g in g_gpu]  # oracle sees exactly the GPU inputs
        inputs = [g.clone() for g in g_cpu]
        o_gpu = gpu.aggregate(g_gpu)
        o_cpu = O.policy_step(ps, g_cpu)
        torch.cuda.synchronize()
        yield t, inputs, [o.float().cpu() for o in o_gpu], o_cpu, [g.float().cpu() for g in g_gpu], g_cpu
        res_gpu = g_gpu


@pytest.mark.slow
@pytest.mark.parametrize("cfg", ["cfg1_1024sq_r1", "cfg2_resnet50_r1", "cfg3_resnet50_r4", "cfg5_lstm_r1_i4"])
def test_baseline_configs_vs_oracle(cfg):
    steps = 3
    for t, inputs, og, oc, rg, rc in _oracle_and_gpu(cfg, steps):
        # step 0 starts from the oracle's own state: per-step bound; later steps free-running
        tol = (TOL_STEP_R1 if CONFIGS[cfg]["rank"] == 1 else TOL_STEP) if t == 0 else TOL_FREE
        for i, g in enumerate(inputs):
            check(_rel(og[i], oc[i], g), tol, cfg, t, i, "out")
            check(_rel(rg[i], rc[i], g), tol, cfg, t, i, "res")


@pytest.mark.slow
def test_baseline_bf16_llama_vs_oracle():
    """cfg4 at full size, two steps: at I = 1 the steps alternate, so step 0 pins the even-start
    form (k_even + reduction + k_apply) and step 1 the odd-start form on the 4096 x 11008 rows
    (odd product + reduction + k_apply, or the fused final pass where the plan takes it)."""
    for t, inputs, og, oc, rg, rc in _oracle_and_gpu("cfg4_llama_r2_bf16", 2, torch.bfloat16):
        for i, g in enumerate(inputs):
            check(_rel(og[i], oc[i], g), TOL_BF16, "cfg4", t, i, "out")
            check(_rel(rg[i], rc[i], g), TOL_BF16, "cfg4", t, i, "res")


@pytest.mark.slow
@pytest.mark.parametrize("rank,iters", [(1, 2), (4, 2), (2, 3)])
def test_resnet50_error_feedback_identity_and_determinism(rank, iters):
    shapes = resnet50_shapes()
    params = [torch.zeros(s, device=DEV) for s in shapes]
    runs = []
    for rep in range(2):
        psgd = PowerSGD(params, Config(rank, 2, iters, 0))
        grads = [torch.from_numpy(f).to(DEV) for f in hash_tensors(shapes, seed=77)]
        orig = [g.clone() for g in grads]
        outs = psgd.aggregate(grads)
        torch.cuda.synchronize()
        for o, a, r in zip(orig, outs, grads):
            check(_rel(a + r, o, o), 1e-6, rank, iters, "ef-identity")
        runs.append(([a.clone() for a in outs], [g.clone() for g in grads],
                     psgd._powersgd._ps_buffer.clone(), psgd._powersgd._qs_buffer.clone()))
    for x, y in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]):
        assert torch.equal(x, y)
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])


@pytest.mark.parametrize("rank", [2, 4, 8, 16, 32])
def test_orthonormal_in_factor_every_rank_bucket(rank):
    """The state P after an even iteration is Householder-orthonormalised; check via the
    next step's behaviour: out is the projection of G onto span(P) at one iteration."""
    shapes = [(300, 200), (64, 1000), (1000, 64)]
    params = [torch.zeros(s, device=DEV) for s in shapes]
    psgd = PowerSGD(params, Config(rank, 0.1, 1, 0))
    p_before = psgd._powersgd._ps_buffer.clone()
    grads = [torch.from_numpy(f).to(DEV) for f in hash_tensors(shapes, seed=5)]
    orig = [g.clone() for g in grads]
    outs = psgd.aggregate(grads)
    torch.cuda.synchronize()
    # oracle from the same state
    ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 0.1, 1, 0)
    ora.codec.p_flat.copy_(p_before.cpu())
    ora.codec.q_flat.copy_(psgd._powersgd._qs_buffer.cpu())  # Q is overwritten anyway at it 0
    oc = O.policy_step(ora, [g.cpu() for g in orig])
    for i, g in enumerate(orig):
        check(_rel(outs[i], oc[i], g), TOL_STEP, rank, i, "out")


@pytest.mark.parametrize("rank,iters", [(12, 2), (16, 2), (16, 3), (32, 2)])
def test_wide_rank_free_running(rank, iters):
    """Ranks 9-32: k_orth_chol16/32 (fp64 MFMA Cholesky-QR) and k_apply's matrix-core tiles
    (apply_tile_mfma, any term count; its fallback loads factor rows per element where m % 4 != 0),
    two free-running steps with error feedback against the oracle from the same initial state."""
    shapes = [(300, 200), (64, 1000), (1000, 64), (128, 8, 3, 3), (40,)]
    params = [torch.zeros(s, device=DEV) for s in shapes]
    psgd = PowerSGD(params, Config(rank, 0.1, iters, 0))
    ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 0.1, iters, 0)
    ora.codec.p_flat.copy_(psgd._powersgd._ps_buffer.cpu())
    ora.codec.q_flat.copy_(psgd._powersgd._qs_buffer.cpu())
    res_d = [torch.zeros(s, device=DEV) for s in shapes]
    res_c = [torch.zeros(s) for s in shapes]
    for t in range(2):
        new = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=60 + t)]
        gd = [r + x.to(DEV) for r, x in zip(res_d, new)]
        gc = [r + x for r, x in zip(res_c, new)]
        scale = [g.cpu().clone() for g in gc]
        od = psgd.aggregate(gd)
        oc = O.policy_step(ora, gc)
        torch.cuda.synchronize()
        for i, g in enumerate(scale):
            check(_rel(od[i], oc[i], g), TOL_FREE, rank, iters, t, i, "out")
            check(_rel(gd[i], gc[i], g), TOL_FREE, rank, iters, t, i, "res")
        res_d, res_c = gd, gc


@pytest.mark.parametrize("rank,wpc,emin", [(1, 1, 16384), (4, 4, 1024), (4, 2, 200000), (2, 3, 4096),
                                         (1, 4, 1024), (4, 3, 16384), (2, 2, 4096), (1, 8, 2048)])
def test_even_segmentation_forms(rank, wpc, emin):
    """The persistent even product (k_even) splits the gradient bytes into ranges, one per
    workgroup (PSGD_EVEN_WPC workgroups per CU, at least PSGD_EVEN_MIN elements each): the
    setting only moves segment boundaries (which rows share a partial). Every setting matches the
    oracle per step from the same state, and a rerun from the same state is bitwise identical."""
    shapes = resnet50_shapes()
    env = {"PSGD_EVEN_WPC": str(wpc), "PSGD_EVEN_MIN": str(emin)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        psgd = PowerSGD([torch.zeros(s, device=DEV) for s in shapes], Config(rank, 2, 2, 0))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    p0 = psgd._powersgd._ps_buffer.clone()
    q0 = psgd._powersgd._qs_buffer.clone()
    grads = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=77)]
    ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 2, 2, 0)
    ora.codec.p_flat.copy_(p0.cpu())
    ora.codec.q_flat.copy_(q0.cpu())
    gc = [g.clone() for g in grads]
    oc = O.policy_step(ora, gc)
    runs = []
    for _ in range(2):
        psgd._powersgd._ps_buffer.copy_(p0)
        psgd._powersgd._qs_buffer.copy_(q0)
        psgd.step_counter = psgd._powersgd.step_counter = 0
        gd = [g.to(DEV) for g in grads]
        od = psgd.aggregate(gd)
        torch.cuda.synchronize()
        runs.append([o.clone() for o in od] + [g.clone() for g in gd] + [psgd._powersgd._qs_buffer.clone()])
        for i, g in enumerate(grads):
            tol = TOL_STEP_R1 if rank == 1 else TOL_STEP
            check(_rel(od[i], oc[i], g), tol, rank, wpc, emin, i, "out")
            check(_rel(gd[i], gc[i], g), tol, rank, wpc, emin, i, "res")
    for x, y in zip(runs[0], runs[1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("rank,dt", [(2, torch.float32), (4, torch.float32), (2, torch.bfloat16),
                                     (4, torch.bfloat16)])
def test_even_full_width_plans(rank, dt):
    """Ranks 2 / 4, fp32 and bf16, at the default k_even workgroups per CU (the instance's
    resident count: 3 at rank 4 fp32, 2 for bf16 rank 2): plans whose every matrix is
    full-width strips (a ragged column count, 700, leaves a partial last strip; a tall-thin
    matrix), then with one narrow matrix added (the narrow-strip path with 3 rows in flight at
    rank 4). One step against the oracle from the same state, and a bitwise rerun."""
    for shapes in ([(512, 1024), (300, 700), (2048, 256)], [(512, 1024), (300, 700), (2048, 256), (96, 40)]):
        psgd = PowerSGD([torch.zeros(s, device=DEV, dtype=dt) for s in shapes], Config(rank, 2, 2, 0))
        p0 = psgd._powersgd._ps_buffer.clone()
        q0 = psgd._powersgd._qs_buffer.clone()
        new = [torch.from_numpy(f) for f in hash_tensors(shapes, seed=91)]
        gin = [g.to(DEV).to(dt) for g in new]
        ora = O.policy_init([torch.zeros(s) for s in shapes], rank, 2, 2, 0)
        ora.codec.p_flat.copy_(p0.cpu())
        ora.codec.q_flat.copy_(q0.cpu())
        gc = [g.float().cpu() for g in gin]
        scale = [g.clone() for g in gc]
        oc = O.policy_step(ora, gc)
        runs = []
        for _ in range(2):
            psgd._powersgd._ps_buffer.copy_(p0)
            psgd._powersgd._qs_buffer.copy_(q0)
            psgd.step_counter = psgd._powersgd.step_counter = 0
            gd = [g.clone() for g in gin]
            od = psgd.aggregate(gd)
            torch.cuda.synchronize()
            runs.append([o.clone() for o in od] + [g.clone() for g in gd])
            tol = TOL_BF16 if dt == torch.bfloat16 else TOL_STEP
            for i, g in enumerate(scale):
                check(_rel(od[i].float(), oc[i], g), tol, rank, str(dt), len(shapes), i, "out")
                check(_rel(gd[i].float(), gc[i], g), tol, rank, str(dt), len(shapes), i, "res")
        for x, y in zip(runs[0], runs[1]):
            assert torch.equal(x, y)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_rank4_projection_wide_rows(dt):
    """The rank-4 projection pass at 256 threads with up to 5 register segments per thread: the
    9c-column rows of the 3x3 convolutions (4608, 2304, 1152, 576 columns: 5 segments of 256,
    128, 64, 32 threads) and a plain 1024-column row, fp32 and bf16, one step against the
    oracle from the same state and a bitwise rerun."""
    shapes = [(512, 4608), (96, 2304), (2048, 1152), (64, 576), (300, 1024)]
    psgd = PowerSGD([torch.zeros(s, device=DEV, dtype=dt) for s in shapes], Config(4, 2, 2, 0))
    p0 = psgd._powersgd._ps_buffer.clone()
    q0 = psgd._powersgd._qs_buffer.clone()
    gin = [torch.from_numpy(f).to(DEV).to(dt) for f in hash_tensors(shapes, seed=97)]
    ora = O.policy_init([torch.zeros(s) for s in shapes], 4, 2, 2, 0)
    ora.codec.p_flat.copy_(p0.cpu())
    ora.codec.q_flat.copy_(q0.cpu())
    gc = [g.float().cpu() for g in gin]
    scale = [g.clone() for g in gc]
    oc = O.policy_step(ora, gc)
    runs = []
    for _ in range(2):
        psgd._powersgd._ps_buffer.copy_(p0)
        psgd._powersgd._qs_buffer.copy_(q0)
        psgd.step_counter = psgd._powersgd.step_counter = 0
        gd = [g.clone() for g in gin]
        od = psgd.aggregate(gd)
        torch.cuda.synchronize()
        runs.append([o.clone() for o in od] + [g.clone() for g in gd] + [psgd._powersgd._qs_buffer.clone(),
                                                                        psgd._powersgd._ps_buffer.clone()])
        tol = TOL_BF16 if dt == torch.bfloat16 else TOL_STEP
        for i, g in enumerate(scale):
            check(_rel(od[i].float(), oc[i], g), tol, str(dt), i, "out")
            check(_rel(gd[i].float(), gc[i], g), tol, str(dt), i, "res")
    for x, y in zip(runs[0], runs[1]):
        assert torch.equal(x, y)
