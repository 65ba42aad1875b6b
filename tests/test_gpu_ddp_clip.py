"""``PowerSGDState(..., max_grad_norm=x)`` under a real ``DistributedDataParallel``: what the hook
hands back in the buckets is clipped by its global L2 norm, in every completion form.

One spawned child, a 1-rank gloo group (DDP needs one) and the stand-in collective library
(tests/stubs/rccl_stub.hip) injected as each state's communicator at world 3 and world 1; the
``_Probe`` models, shapes and ~10 KB buckets of tests/test_gpu_ddp_direct.py (loss sum_i <p_i, c_i>:
the local gradient of p_i is exactly c_i). Four steps: DDP rebuilds its buckets after the first, and
both step parities run. Gradients grow 2 x per step and the threshold is the norm of step 1's
unclipped averages, so step 0 does not clip and steps 2 and 3 do.

Models: (a) three stages + ``max_grad_norm``; (b) ``direct_store`` + ``max_grad_norm`` (the one-call
completion followed by psgd_clip_dst); (c) three stages unclipped, then
``torch.nn.utils.clip_grad_norm_`` on the gradients. (b) is defined as (a): raw bits. (a) against
(c): the library's norm on a compressing step comes from the low-rank factors and may differ from
the norm of the stored averages by the project's per-step tolerance, 1e-5 x the norm of the step's
input gradients (tests/test_gpu_clip.py); call that `bound`. The coefficient x / (norm + 1e-6)
then differs from torch's by at most bound / norm relative, and each clipped element |u| coef by
that plus the roundings of both sides (torch: an fp32 norm, about 2^-23 relative, an fp32
coefficient and product, 2^-24 each; the library: float(coef) and the product, 2^-24 each; under
2^-22 together): |a - c| <= |u| (bound / norm + 2^-22) with u the unclipped value of a twin. A
warm-up step's norm is the stream form's: against the fp64 norm of the twin's averages at 1e-10
relative (the bound of tests/test_gpu_clip.py for that form)."""
import math
import os

import pytest
import torch

from test_gpu_ddp_direct import SHAPES, STEPS, STUB, _Probe, _bits, _fresh, _init, _mcr

pytestmark = pytest.mark.gpu


def _norm64(ts):
    return math.sqrt(sum(float((t.double() ** 2).sum()) for t in ts))


class _Child:
    def __init__(self, init):
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)

    def model(self, cfg, world, dtype=torch.float32, direct=False, **kw):
        """A DDP model with the hook and the stand-in communicator of `world`; `kw` goes to the state."""
        from torch.nn.parallel import DistributedDataParallel as DDP

        from powersgd_amd import _lib
        from powersgd_amd.ddp import PowerSGDState, powersgd_hook

        gen = torch.Generator().manual_seed(7)
        net = _Probe([torch.randn(s, generator=gen).to(dtype) for s in SHAPES]).to(self.dev)
        ddp = DDP(net, device_ids=[0], bucket_cap_mb=0.01)
        state = PowerSGDState(cfg, params=list(net.parameters()), **kw)
        if direct:
            state.direct_store = True
        state.powersgd._powersgd._comm = _lib.Comm(world, 0, _lib.comm_unique_id(), 0)
        ddp.register_comm_hook(state, powersgd_hook)
        return ddp, state

    def run(self, ddp, state, t, dtype=torch.float32):
        """One backward of step t; the gradients the hook handed back (clones) and the inputs."""
        cs = [g.to(self.dev).to(dtype) for g in _fresh(t)]
        ddp(cs).backward()
        torch.cuda.synchronize()
        params = list(ddp.module.parameters())
        grads = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        return grads, cs

    def unclipped(self, cfg, world, dtype=torch.float32, **kw):
        """The unclipped twin: per step its gradients, the fp64 norm of them and of the inputs."""
        ddp, state = self.model(cfg, world, dtype, **kw)
        rec = []
        for t in range(STEPS):
            grads, cs = self.run(ddp, state, t, dtype)
            rec.append({"u": grads, "norm": _norm64(grads), "input": _norm64(cs)})
        assert state.last_grad_norm is None and state.last_clip_coef is None and state.max_grad_norm is None
        state.powersgd.close()
        return rec

    def close(self):
        torch.distributed.destroy_process_group()


def _state_bits(state):
    codec = state.powersgd._powersgd
    return {"residual": _bits(state.residual.float()) if state.residual.dtype != torch.float32 else _bits(state.residual),
            "ps": _bits(codec._ps_buffer), "qs": _bits(codec._qs_buffer)}


def _equal_states(sa, sb, ga, gb, ctx, results=True):
    for i, (p, q) in enumerate(zip(ga, gb)):
        assert torch.equal(p.view(torch.uint8), q.view(torch.uint8)), (ctx, i, "p.grad")
    a, b = _state_bits(sa), _state_bits(sb)
    for k in a:
        assert torch.equal(a[k], b[k]), (ctx, k)
    if results:
        for x, y in ((sa.last_grad_norm, sb.last_grad_norm), (sa.last_clip_coef, sb.last_clip_coef)):
            assert x.dim() == 0 and x.dtype == torch.float64 and x.is_cuda
            assert torch.equal(x.view(torch.int64), y.view(torch.int64)), (ctx, float(x), float(y))


# ------------------------------------------------------------------ test 1
def _three_forms(_, init):
    from powersgd_amd import Config

    ch = _Child(init)
    try:
        for world, rank in ((3, 1), (3, 4), (3, 16), (1, 1), (1, 4), (1, 16)):
            iters = 2
            cfg = Config(rank, _mcr(rank, iters), iters, 0)
            twin = ch.unclipped(cfg, world)
            thr = twin[1]["norm"]
            assert twin[0]["norm"] < thr < twin[2]["norm"] < twin[3]["norm"], [r["norm"] for r in twin]
            a_ddp, a = ch.model(cfg, world, max_grad_norm=thr)
            b_ddp, b = ch.model(cfg, world, direct=True, max_grad_norm=thr)
            assert a.max_grad_norm == b.max_grad_norm == thr
            assert a.last_grad_norm is None and b.last_clip_coef is None
            for t in range(STEPS):
                ctx = (world, rank, t)
                assert b.direct_store_applies() is True, ctx
                assert a.direct_store_applies() is False, ctx
                ga, cs = ch.run(a_ddp, a, t)
                gb, _ = ch.run(b_ddp, b, t)
                _equal_states(a, b, ga, gb, ctx)  # (b) is (a), bit for bit
                # (a) against (c): torch's clip of the unclipped twin's gradients
                u = twin[t]["u"]
                c = [torch.nn.Parameter(torch.empty_like(x)) for x in u]
                for p, x in zip(c, u):
                    p.grad = x.clone()
                tnorm = float(torch.nn.utils.clip_grad_norm_(c, thr))
                norm, coef = float(a.last_grad_norm), float(a.last_clip_coef)
                bound = 1e-5 * twin[t]["input"]
                print(f"ddp clip world={world} rank={rank} step={t}: norm {norm:.9g} torch {tnorm:.9g} "
                      f"|diff| / bound = {abs(norm - twin[t]['norm']) / bound:.3e}, coef {coef:.9g}")
                assert abs(norm - twin[t]["norm"]) <= bound, ctx
                assert abs(norm - tnorm) <= bound + 2.0 ** -22 * tnorm, ctx
                if t == 0:
                    assert coef == 1.0, ctx
                    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(ga, u)), ctx
                if t >= 2:
                    assert coef < 1.0, ctx
                    assert abs(coef - thr / (norm + 1e-6)) <= 1e-15, ctx
                    assert any(not torch.equal(x, y) for x, y in zip(ga, u)), ctx
                rel = bound / twin[t]["norm"] + 2.0 ** -22
                for i, (x, p, y) in enumerate(zip(ga, c, u)):
                    assert bool(((x - p.grad).abs() <= y.abs() * rel).all()), (ctx, i)
                # the residual is the unclipped flow's: clipping never touches it
            assert b.last_grad_norm is b.powersgd.last_grad_norm and b._clip_result is b.powersgd._clip_result
            a.powersgd.close()
            b.powersgd.close()
    finally:
        ch.close()


def test_direct_and_three_stage_clip_agree_bitwise_and_match_torch(tmp_path):
    """Ranks 1 / 4 / 16 at I = 2, world 3 and a 1-rank communicator, four steps."""
    torch.multiprocessing.spawn(_three_forms, args=(_init(tmp_path),), nprocs=1, join=True)


# ------------------------------------------------------------------ test 2
def _other_forms(_, init):
    from powersgd_amd import Config

    ch = _Child(init)
    try:
        # bf16 parameters over an fp32 residual: fused=True with max_grad_norm runs the three stages
        bf = torch.bfloat16
        cfg = Config(4, _mcr(4, 2), 2, 0)
        kw = dict(dtype=bf, residual_dtype=torch.float32)
        probe_ddp, probe = ch.model(cfg, 3, fused=True, **kw)
        assert probe.fused_folds() == (0, 1)  # the plan is one the fused form serves when nothing clips
        probe.max_grad_norm = 1.0
        assert probe.fused_folds() == (0, 0)
        probe.powersgd.close()
        m_ddp, m = ch.model(cfg, 3, max_grad_norm=math.inf, **kw)
        norms = []
        for t in range(STEPS):
            ch.run(m_ddp, m, t, bf)
            norms.append(float(m.last_grad_norm))
            assert float(m.last_clip_coef) == 1.0
        m.powersgd.close()
        thr = norms[1]
        assert norms[0] < thr < norms[2] < norms[3], norms
        f_ddp, f = ch.model(cfg, 3, fused=True, max_grad_norm=thr, **kw)
        p_ddp, p = ch.model(cfg, 3, fused=False, max_grad_norm=thr, **kw)
        for t in range(STEPS):
            assert f.fused_folds() == (0, 0) and p.fused_folds() == (0, 0), t
            gf, _ = ch.run(f_ddp, f, t, bf)
            gp, _ = ch.run(p_ddp, p, t, bf)
            assert all(g.dtype == bf for g in gf)
            _equal_states(f, p, gf, gp, ("bf16 fused", t))
            assert (float(f.last_clip_coef) == 1.0) if t == 0 else (float(f.last_clip_coef) < 1.0 or t == 1), t
        f.powersgd.close()
        p.powersgd.close()

        # a warm-up step clips through the same call (stream form): its norm against the fp64 norm of
        # the twin's averages, in both completion forms; direct_store starts with the first compressing step
        cfg = Config(2, _mcr(2, 2), 2, 1)
        twin = ch.unclipped(cfg, 3)
        thr = twin[0]["norm"] / 2
        a_ddp, a = ch.model(cfg, 3, max_grad_norm=thr)
        b_ddp, b = ch.model(cfg, 3, direct=True, max_grad_norm=thr)
        for t in range(STEPS):
            assert b.direct_store_applies() is (t >= 1), t
            ga, _ = ch.run(a_ddp, a, t)
            gb, _ = ch.run(b_ddp, b, t)
            _equal_states(a, b, ga, gb, ("warm-up", t))
            if t == 0:
                norm, want = float(a.last_grad_norm), twin[0]["norm"]
                print(f"ddp clip warm-up: rel err {abs(norm - want) / want:.3e}")
                assert abs(norm - want) <= 1e-10 * want
                assert abs(float(a.last_clip_coef) - thr / (norm + 1e-6)) <= 1e-15
                coef32 = torch.tensor(float(a.last_clip_coef), dtype=torch.float32)
                for x, y in zip(ga, twin[0]["u"]):
                    assert torch.equal(x.cpu(), y.cpu() * coef32)
        a.powersgd.close()
        b.powersgd.close()

        # max_grad_norm=None: the parent's code path, nothing reported
        cfg = Config(4, _mcr(4, 2), 2, 0)
        for direct in (False, True):
            n_ddp, n = ch.model(cfg, 3, direct=direct, max_grad_norm=None)
            k_ddp, k = ch.model(cfg, 3, direct=direct)
            for t in range(STEPS):
                gn, _ = ch.run(n_ddp, n, t)
                gk, _ = ch.run(k_ddp, k, t)
                _equal_states(n, k, gn, gk, ("None", direct, t), results=False)
                assert n.last_grad_norm is None and n.last_clip_coef is None and n.max_grad_norm is None
            # settable afterwards, validated as at construction
            n.max_grad_norm = 0.5
            assert n.max_grad_norm == 0.5 and n.powersgd.max_grad_norm == 0.5
            with pytest.raises(ValueError, match="max_grad_norm must be a positive number or None"):
                n.max_grad_norm = -1.0
            n.powersgd.close()
            k.powersgd.close()
    finally:
        ch.close()


def test_fused_warmup_and_default_forms(tmp_path):
    """bf16 with ``fused=True``: the three stages while clipping, bit for bit ``fused=False``; a warm-up
    step clips through the stream form; ``max_grad_norm=None`` is the state without the keyword."""
    torch.multiprocessing.spawn(_other_forms, args=(_init(tmp_path),), nprocs=1, join=True)
