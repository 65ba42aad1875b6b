"""GPU parity of the seam descriptors (RedSeam beside each reduction item, FinRng beside each
fused row block; powersgd_amd/csrc/psgd_internal.h): the rank-1 norm folds of k_reduce and of
the fused final passes take their sum-of-squares ranges and factor offsets from these lists
instead of through MatDesc and the per-group range tables.

Every case runs two steps through PowerSGD.aggregate at world size 1, each from the oracle's own
state and residual, against the CPU oracle at the per-step tolerances of tests/test_gpu_parity.py
(1e-6 at rank 1, 1e-5 at ranks 2 and 4, 4e-3 for bf16 gradients), reruns the step from the same
state and asks for bitwise equal outputs, residuals and P/Q state, and runs the same step in the
world-size > 1 call sequence (psgd_compress per iteration, psgd_decompress) at world size 1 against
the same oracle values.

The shapes are the smallest that make each field matter:
* three equal [24, 40] matrices form one rank-1 group beside two single-matrix groups: the joint
  norm N of the group differs from a member's c, and the group's item range from the matrix's;
* [32, 771]: a Q panel over several reduction items with a ragged last one (771 = 3 * 257 columns,
  771 % 4 != 0);
* [4096, 32]: a tall, narrow matrix of one column strip; the plans are created with
  PSGD_EVEN_MIN=1024 (at least that many gradient elements per k_even workgroup, as
  tests/test_gpu_parity.py::test_even_segmentation_forms sets it), which cuts the strip into about
  128 segments, more than kRedWide = 64 partials per element, so its even items hold one element
  per lane (RedItem::per = 1). 4096 rows is the row count of the LSTM baseline config, which the
  suite holds to 1e-6 at rank 1; a [70000, 16] matrix (also more than 64 odd-even row blocks)
  misses that bound by the summation order of its 70000-term column sums alone (1.8e-6 measured,
  fp32 against the CPU oracle), so it is not used;
* a 1-D tensor stays uncompressed: its flat-pack items lead the final launch, ahead of the row
  blocks the FinRng list is indexed by.
Iterations: I = 2 (projection form; ranks 2 and 4 with the folded Gram), I = 3 and I = 4 (odd-even
pass and K-term final pass), I = 1 (k_apply after the iteration-0 fold).
"""
import os

import pytest
import torch

from oracle import powersgd_oracle as O
from powersgd_amd import Config, PowerSGD
from powersgd_amd.workloads import hash_tensors

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_STEP = 1e-5
TOL_STEP_R1 = 1e-6
TOL_BF16 = 4e-3

SHAPES = [(24, 40), (24, 40), (24, 40), (48, 24), (64, 32), (32, 771), (4096, 32), (40,)]
MCR = 2

CASES = [
    (1, 2, torch.float32),
    (2, 2, torch.float32),
    (4, 2, torch.float32),
    (1, 3, torch.float32),
    (1, 4, torch.float32),
    (1, 1, torch.float32),
    (2, 2, torch.bfloat16),
]


def _rel(a, b, scale):
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(float(scale.double().norm()), 1e-30)


def _set_state(psgd, p, q, step):
    psgd._powersgd._ps_buffer.copy_(p)
    psgd._powersgd._qs_buffer.copy_(q)
    psgd.step_counter = psgd._powersgd.step_counter = step


def _split_step(psgd, grads, step, dtype):
    """The world-size > 1 call sequence at world size 1; returns the outputs per tensor."""
    codec = psgd._powersgd
    stream = torch.cuda.current_stream().cuda_stream
    mask = psgd.is_compressed_mask
    codec._table.fill([g for g, m in zip(grads, mask) if m])
    ptrs = codec._table.comp_addr()
    out = torch.empty(codec._out_numel, device=DEV, dtype=dtype)
    for it in range(psgd.config.num_iters_per_step):
        codec._plan.compress(ptrs, step, it, stream)
    codec._plan.decompress(ptrs, out.data_ptr(), step, 1, stream)
    unc = iter(psgd._allreduce.aggregate([g for g, m in zip(grads, mask) if not m]))
    torch.cuda.synchronize()
    offs = iter(codec._plan.output_offsets())
    outs = []
    for g, m in zip(grads, mask):
        if m:
            o = next(offs)
            outs.append(out[o:o + g.numel()].view(g.shape).clone())
        else:
            outs.append(next(unc).clone())
    return outs


@pytest.mark.parametrize("rank,iters,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_seam_descriptors(rank, iters, dtype):
    tol = TOL_BF16 if dtype == torch.bfloat16 else TOL_STEP_R1 if rank == 1 else TOL_STEP
    old = os.environ.get("PSGD_EVEN_MIN")
    os.environ["PSGD_EVEN_MIN"] = "1024"  # read once, at plan creation
    try:
        psgd = PowerSGD([torch.zeros(s, device=DEV, dtype=dtype) for s in SHAPES], Config(rank, MCR, iters, 0))
    finally:
        if old is None:
            del os.environ["PSGD_EVEN_MIN"]
        else:
            os.environ["PSGD_EVEN_MIN"] = old
    assert psgd.is_compressed_mask == [True] * (len(SHAPES) - 1) + [False]
    ora = O.policy_init([torch.zeros(s) for s in SHAPES], rank, MCR, iters, 0)
    ora.codec.p_flat.copy_(psgd._powersgd._ps_buffer.cpu())
    ora.codec.q_flat.copy_(psgd._powersgd._qs_buffer.cpu())
    res = [torch.zeros(s) for s in SHAPES]
    for t in range(2):
        fresh = [torch.from_numpy(f) for f in hash_tensors(SHAPES, seed=300 + t)]
        gin = [(r + f).to(DEV).to(dtype) for r, f in zip(res, fresh)]
        x = [g.float().cpu() for g in gin]  # the oracle sees exactly the GPU's inputs
        p0, q0 = ora.codec.p_flat.clone().to(DEV), ora.codec.q_flat.clone().to(DEV)
        g_c = [g.clone() for g in x]
        o_c = O.policy_step(ora, g_c)
        runs = []
        for _ in range(2):  # the step, and its rerun from the same state
            _set_state(psgd, p0, q0, t)
            gd = [g.clone() for g in gin]
            od = psgd.aggregate(gd)
            torch.cuda.synchronize()
            runs.append([o.clone() for o in od] + gd +
                        [psgd._powersgd._ps_buffer.clone(), psgd._powersgd._qs_buffer.clone()])
        od, gd = runs[0][:len(SHAPES)], runs[0][len(SHAPES):2 * len(SHAPES)]
        errs = []
        for i in range(len(SHAPES)):
            errs.append((_rel(od[i].float(), o_c[i], x[i]), _rel(gd[i].float(), g_c[i], x[i])))
        print(f"rank {rank} I {iters} {dtype} step {t}: max out/res error "
              f"{max(e[0] for e in errs):.3g} / {max(e[1] for e in errs):.3g} (bound {tol:g})")
        for i, (eo, er) in enumerate(errs):
            assert eo <= tol and er <= tol, (rank, iters, t, i, SHAPES[i], eo, er)
        for a, b in zip(runs[0], runs[1]):
            assert torch.equal(a, b), (rank, iters, t, "rerun differs")
        # the same step as psgd_compress x I + psgd_decompress
        _set_state(psgd, p0, q0, t)
        gs = [g.clone() for g in gin]
        os_ = _split_step(psgd, gs, t, dtype)
        for i in range(len(SHAPES)):
            eo, er = _rel(os_[i].float(), o_c[i], x[i]), _rel(gs[i].float(), g_c[i], x[i])
            assert eo <= tol and er <= tol, (rank, iters, t, i, SHAPES[i], "split", eo, er)
        res = g_c
