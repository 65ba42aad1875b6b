"""``PowerSGDState(..., residual_dtype=torch.float32, fused=True)`` at rank 16 under a real
``DistributedDataParallel`` against ``fused=False`` on the same build: the one-call completion
(psgd_aggregate_mixed_comm_dst: the codec's matrix-core final pass stores the bf16 averages into
the DDP buckets' gradient views) is defined as the three stages it replaces, so everything is
compared with ``torch.equal`` on raw bits.

One spawned child, a 1-rank gloo group (DDP needs one), and the stand-in collective library
(tests/stubs/rccl_stub.hip) injected as each state's communicator at world 3 and world 1, as
tests/test_gpu_ddp_fused.py sets it up. Two ``_Probe`` models (loss sum_i <p_i, c_i>: the local
gradient of p_i is exactly c_i) over the shapes of tests/test_gpu_mixed_mfma.py plus (41,), so that
later parameters sit at odd element offsets of their ~10 KB buckets. Three steps: DDP rebuilds its
buckets after the first."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "stubs", "librccl_stub.so")
BF16 = torch.bfloat16
SHAPES = [(300, 520), (300, 520), (24, 136), (130, 67), (64, 3, 3, 3), (40,), (257, 260), (1, 96), (96, 1), (41,)]
STEPS = 3
RANK = 16


def _fresh(t: int):
    """Seeded bf16 gradients of step t whose scale grows each step; a few -0.0 among them."""
    gen = torch.Generator().manual_seed(1000 + t)
    out = []
    for s in SHAPES:
        g = (torch.randn(s, generator=gen) * float(2 ** t)).to(BF16)
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
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


class _Child:
    def __init__(self, init):
        os.environ["PSGD_RCCL_LIB_FORCE"] = STUB
        os.environ["PSGD_TESTING"] = "1"  # the override's second opt-in (psgd_comm.cpp)
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        torch.distributed.init_process_group("gloo", init_method=init, rank=0, world_size=1)

    def model(self, cfg, fused, world, ptrs):
        """A DDP model with the hook and the stand-in communicator of `world`. `ptrs` collects the
        address of every gradient view the hook is handed."""
        from torch.nn.parallel import DistributedDataParallel as DDP

        from powersgd_amd import _lib
        from powersgd_amd.ddp import PowerSGDState, powersgd_hook

        gen = torch.Generator().manual_seed(7)
        net = _Probe([torch.randn(s, generator=gen).to(BF16) for s in SHAPES]).to(self.dev)
        ddp = DDP(net, device_ids=[0], bucket_cap_mb=0.01)
        state = PowerSGDState(cfg, params=list(net.parameters()), residual_dtype=torch.float32, fused=fused)
        state.powersgd._powersgd._comm = _lib.Comm(world, 0, _lib.comm_unique_id(), 0)
        mask = state.powersgd.is_compressed_mask
        for s, c in zip(SHAPES, mask):
            assert c or len(s) == 1 or 1 in s, (s, "both matrix dimensions above 1: compressed")
        assert not mask[SHAPES.index((40,))], mask

        def hook(st, bucket):
            ptrs.extend(g.data_ptr() for g in bucket.gradients())
            return powersgd_hook(st, bucket)

        ddp.register_comm_hook(state, hook)
        return ddp, state

    def compare(self, cfg, world, ctx):
        """STEPS backward passes of a fused and an unfused model on the same inputs; after each,
        every observable of the two must agree bit for bit. Returns the fused model's destination
        addresses."""
        ptrs, other = [], []
        fused, fs = self.model(cfg, True, world, ptrs)
        plain, ps = self.model(cfg, False, world, other)
        assert torch.equal(fs.powersgd._powersgd._ps_buffer, ps.powersgd._powersgd._ps_buffer)
        for t in range(STEPS):
            cs = [g.to(self.dev) for g in _fresh(t)]
            assert fs.fused_folds() == (0, 1), (ctx, t, fs.fused_folds())
            assert ps.fused_folds() == (0, 0), (ctx, t)
            for ddp in (fused, plain):
                ddp(cs).backward()
                torch.cuda.synchronize()
            pf, pp = list(fused.module.parameters()), list(plain.module.parameters())
            for i in range(len(SHAPES)):
                assert pf[i].grad.dtype == BF16
                assert torch.equal(_bits(pf[i].grad), _bits(pp[i].grad)), (ctx, t, i, "p.grad")
                assert torch.equal(_bits(fs.views[i]), _bits(ps.views[i])), (ctx, t, i, "residual")
            cf, cp = fs.powersgd._powersgd, ps.powersgd._powersgd
            assert torch.equal(_bits(cf._ps_buffer), _bits(cp._ps_buffer)), (ctx, t, "P")
            assert torch.equal(_bits(cf._qs_buffer), _bits(cp._qs_buffer)), (ctx, t, "Q")
            assert fs.powersgd.step_counter == ps.powersgd.step_counter == t + 1
            assert cf.step_counter == cp.step_counter
            assert any(bool(v.any()) for v in fs.views), (ctx, t)  # a non-trivial residual
            for p in pf + pp:
                p.grad = None
        fs.powersgd.close()
        ps.powersgd.close()
        return ptrs

    def close(self):
        torch.distributed.destroy_process_group()


def _init(tmp_path):
    return f"file://{tmp_path}/store"


def _fused_vs_unfused(_, init):
    from powersgd_amd import Config

    ch = _Child(init)
    try:
        odd = 0
        for world in (3, 1):
            for iters in (1, 2):
                ptrs = ch.compare(Config(RANK, 1.5 / iters, iters, 0), world, (world, iters))
                odd += sum(p % 4 == 2 for p in ptrs)
        # some averages were stored at destinations that are 2-byte aligned only
        assert odd > 0
    finally:
        ch.close()


def test_real_ddp_fused_equals_unfused_bitwise(tmp_path):
    """Rank 16 x 1-2 iterations at world 3 and on a 1-rank communicator, three steps (DDP's bucket
    rebuild included); ``fused_folds()`` is (0, 1) on every step."""
    torch.multiprocessing.spawn(_fused_vs_unfused, args=(_init(tmp_path),), nprocs=1, join=True)
