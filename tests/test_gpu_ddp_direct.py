"""``PowerSGDState.direct_store = True`` under a real ``DistributedDataParallel`` against a plain
state on the same build: the one-call completion (psgd_aggregate_comm_dst: the codec's final pass
stores the fp32 averages into the DDP buckets' gradient views) is defined as the three stages it
replaces, so everything is compared with ``torch.equal`` on raw bits.

One spawned child, a 1-rank gloo group (DDP needs one), and the stand-in collective library
(tests/stubs/rccl_stub.hip) injected as each state's communicator at world 3 and world 1, as
tests/test_gpu_ddp_fused.py sets it up. Two ``_Probe`` models (loss sum_i <p_i, c_i>: the local
gradient of p_i is exactly c_i) over the shapes of tests/test_gpu_comm_dst.py plus (41,), so that
later parameters sit at offsets of their ~10 KB buckets that are no multiple of 4 elements. Four
steps: DDP rebuilds its buckets after the first (a changed bucket layout), and both step parities run."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
SHAPES = [(128, 64, 3, 3), (256, 300), (96, 200), (64, 100), (50, 150), (33, 65), (7, 5), (40,), (97,), (1,), (41,)]
STEPS = 4


def _rate(shape, rank, iters):
    sh = list(shape)
    return torch.Size(sh).numel() / (0.5 * iters * min(rank, min(sh)) * sum(sh))


def _mcr(rank, iters):
    # 0.99 x the smallest rate of a 2-D shape: every 2-D shape compresses, (40,), (41,), (97,) never do
    return 0.99 * min(_rate(s, rank, iters) for s in SHAPES if len(s) > 1)


def _fresh(t):
    """Seeded gradients of step t whose scale grows each step; a few -0.0 among them."""
    gen = torch.Generator().manual_seed(4000 + t)
    out = []
    for s in SHAPES:
        g = torch.randn(s, generator=gen) * float(2 ** t)
        g.view(-1)[::7] = -0.0
        out.append(g)
    return out


class _Probe(torch.nn.Module):
    def __init__(self, init):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.clone()) for p in init])

    def forward(self, cs):
        return sum((p * c).sum() for p, c in zip(self.ps, cs))


def _bits(x):
    return x.contiguous().view(torch.int32)


class _Child:
    def __init__(self, init):
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)
        self.stub = ctypes.CDLL(STUB)  # the same handle the library opened: one call counter
        self.stub.psgd_stub_calls.restype = ctypes.c_longlong

    def model(self, cfg, direct, world, ptrs):
        """A DDP model with the hook; `world`: the stand-in communicator's (None: none injected, the
        plain gloo group). `ptrs` collects (bucket base, view address) of every gradient view the
        hook is handed."""
        from torch.nn.parallel import DistributedDataParallel as DDP

        from powersgd_amd import _lib
        from powersgd_amd.ddp import PowerSGDState, powersgd_hook

        gen = torch.Generator().manual_seed(7)
        net = _Probe([torch.randn(s, generator=gen) for s in SHAPES]).to(self.dev)
        ddp = DDP(net, device_ids=[0], bucket_cap_mb=0.01)
        state = PowerSGDState(cfg, params=list(net.parameters()))
        assert state.direct_store is False  # the default
        state.direct_store = direct
        if world is not None:
            state.powersgd._powersgd._comm = _lib.Comm(world, 0, _lib.comm_unique_id(), 0)

        def hook(st, bucket):
            ptrs.append(tuple(g.data_ptr() for g in bucket.gradients()))
            return powersgd_hook(st, bucket)

        ddp.register_comm_hook(state, hook)
        return ddp, state

    def compare(self, cfg, world, want, ctx):
        """STEPS backward passes of a direct-store and a plain model on the same inputs; after each,
        every observable of the two must agree bit for bit. `want[t]`: direct_store_applies() before
        step t. Returns the direct model's per-bucket view addresses, hook call by hook call."""
        ptrs, other = [], []
        direct, ds = self.model(cfg, True, world, ptrs)
        plain, ps = self.model(cfg, False, world, other)
        assert torch.equal(ds.powersgd._powersgd._ps_buffer, ps.powersgd._powersgd._ps_buffer)
        for t in range(STEPS):
            cs = [g.to(self.dev) for g in _fresh(t)]
            assert ds.direct_store_applies() is want[t], (ctx, t, ds.direct_store_applies())
            assert ps.direct_store_applies() is False, (ctx, t)
            calls = []
            for ddp in (direct, plain):
                n0 = self.stub.psgd_stub_calls()
                ddp(cs).backward()
                torch.cuda.synchronize()
                calls.append(self.stub.psgd_stub_calls() - n0)
            assert calls[0] == calls[1], (ctx, t, calls)
            if world is not None and want[t]:
                # one collective per power iteration, the flat tail grouped with the last one
                assert calls[0] == cfg.num_iters_per_step + 1, (ctx, t, calls)
            pd, pp = list(direct.module.parameters()), list(plain.module.parameters())
            for i in range(len(SHAPES)):
                assert torch.equal(_bits(pd[i].grad), _bits(pp[i].grad)), (ctx, t, i, "p.grad")
                assert torch.equal(_bits(ds.views[i]), _bits(ps.views[i])), (ctx, t, i, "residual")
            cd, cp = ds.powersgd._powersgd, ps.powersgd._powersgd
            assert torch.equal(_bits(cd._ps_buffer), _bits(cp._ps_buffer)), (ctx, t, "P")
            assert torch.equal(_bits(cd._qs_buffer), _bits(cp._qs_buffer)), (ctx, t, "Q")
            assert ds.powersgd.step_counter == ps.powersgd.step_counter == t + 1
            assert cd.step_counter == cp.step_counter
            if want[t]:  # a compressing step leaves a non-trivial residual
                assert any(bool(v.any()) for v in ds.views), (ctx, t)
            for p in pd + pp:
                p.grad = None
        with pytest.raises(ValueError, match="before the first backward"):
            ds.direct_store = False
        ds.powersgd.close()
        ps.powersgd.close()
        return ptrs

    def close(self):
        torch.distributed.destroy_process_group()


def _init(tmp_path):
    return f"file://{tmp_path}/store"


def _direct_vs_plain(_, init):
    from powersgd_amd import Config

    ch = _Child(init)
    try:
        unaligned, relaid = 0, 0
        for world, rank, iters in ((3, 1, 1), (3, 2, 2), (3, 4, 3), (3, 8, 1), (3, 16, 2), (3, 32, 1),
                                   (1, 1, 2), (1, 2, 1), (1, 16, 1)):
            cfg = Config(rank, _mcr(rank, iters), iters, 0)
            ptrs = ch.compare(cfg, world, [True] * STEPS, (world, rank, iters))
            unaligned += sum(p % 16 != 0 for call in ptrs for p in call)
            per_step = len(ptrs) // STEPS
            relaid += ptrs[:per_step] != ptrs[per_step:2 * per_step]
        # some averages were stored at destinations that are not 16-byte aligned, and the bucket
        # layout changed after the first iteration (DDP's rebuild)
        assert unaligned > 0
        assert relaid > 0
    finally:
        ch.close()


def test_real_ddp_direct_equals_plain_bitwise(tmp_path):
    """Rank buckets 1-32 at world 3 and on a 1-rank communicator, four steps (DDP's bucket rebuild
    and both step parities included)."""
    torch.multiprocessing.spawn(_direct_vs_plain, args=(_init(tmp_path),), nprocs=1, join=True)


def _fallbacks(_, init):
    from powersgd_amd import Config

    ch = _Child(init)
    try:
        # a warm-up step runs the three stages; the first compressing step takes the one-call form
        ch.compare(Config(2, _mcr(2, 2), 2, 1), 3, [False, True, True, True], "warm-up")
        # a plan with an instance that is not admitted (rank bucket 8, two iterations)
        ch.compare(Config(8, _mcr(8, 2), 2, 0), 3, [False] * STEPS, "rank 8, I = 2")
        # a plain gloo group: no communicator of the library's, the three stages throughout
        ch.compare(Config(2, _mcr(2, 2), 2, 0), None, [False] * STEPS, "gloo")
    finally:
        ch.close()


def test_fallbacks_run_the_three_stages(tmp_path):
    """A warm-up step (``start_compressing_after_num_steps=1``), a plan the call refuses and a plain
    gloo group: ``direct_store_applies()`` is False there and the run equals the plain one."""
    torch.multiprocessing.spawn(_fallbacks, args=(_init(tmp_path),), nprocs=1, join=True)
