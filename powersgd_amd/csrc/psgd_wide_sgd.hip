// The final pass of psgd_aggregate_comm_sgd_wide (psgd_onecall.cpp): effective ranks 33-128, with the
// SGD step applied where k_wide_apply<float> would have stored the fp32 average. Its master-weight
// form, k_wide_apply_sgd_mp, is psgd_wide_sgd_mp.hip; the epilogue both share is psgd_wide_sgd.cuh.
//
//   k_wide_apply_sgd<R, SHARED>   residual = G_0 - sum_k P_k Q_k^T (fp32, in place),
//                                 g = alpha sum_k Pbar_k Qbar_k^T, never stored:
//                                 (p, buf) <- THE UPDATE(g, p, buf) of psgd_sgd_hyper
//
// Tile, accumulators, MFMA sequence and operand movement are wide_pass's (psgd_wide_pass.cuh) as
// they stand: the 64-row x 256-column tile, 16 rows per wave, four 64-column steps; the Q-side
// blocks staged once per workgroup in LDS (row stride R + 4 floats, two buffers, the next block's
// global loads ahead of the current MFMA chain, one barrier per block), the P side once per tile
// in registers. Every accumulator receives k_wide_apply<float>'s sequence, so the residual and
// g = acc x alpha (that kernel's one fp32 multiply; at world size 1 the sums themselves) have its
// bits, and sgd_update (psgd_stream.cuh) is the device function of k_sgd_update: the fused step
// equals psgd_aggregate_comm followed by psgd_sgd_update bit for bit. g is pinned as a rounded
// value of its own before the update, so no product alpha x acc is contracted into the update's
// first add (d = g + weight_decay x p).
//
// The epilogue. A lane owns, per column step, four row quads (u = 0 .. 3) of its row: columns
// sbeg + 64 step + 16 u + 4 kq .. + 3, read and written at the same element of the tensor's own p
// and buf (pointer tables indexed by MatDesc::tensor).
//   two bodies     a tensor's momentum buffer may be absent (momentum == 0: the table entry is NULL
//                  or a placeholder). The tile picks one of two bodies once, from the record
//                  (workgroup-uniform, a scalar branch): sgd_epilogue<true> moves p and buf,
//                  sgd_epilogue<false> has no buf operand at all. The p stream runs alone there
//                  because no instruction on buf exists in that body, not because one is masked
//                  off; neither its pointer nor its alignment is looked at.
//   in flight      the quads of one column step are 32 VGPRs with momentum (p and buf), 16 without.
//                  With momentum the requests of steps s + 1 and s + 2 are issued before the update
//                  and the stores of step s: a ring of three steps, 96 VGPRs beside the 64
//                  accumulator VGPRs, the envelope k_wide_apply_adam's two steps of 48 hold at two
//                  waves per SIMD, and one more step of latency covered for the same registers
//                  (vmcnt retires in order: waiting for the quads of step s + 2 does not wait for
//                  the stores of steps s and s + 1).
//                  Without momentum all four steps' p quads (64 VGPRs) are requested before the
//                  first update: the whole tile's reads are in flight at once. The P quads and the
//                  staging prefetch of the pass (up to 64 VGPRs at R = 128) are dead by then. None
//                  is requested while an LDS block is in flight: the first request follows the last
//                  pass. Addresses are formed at use (fresh()), none lives across a pass.
//                  profiles/sgd_wide/resources.txt: all four instances hold two waves per SIMD
//                  without scratch at these depths.
//   access width   16 bytes where m % 4 == 0 and p (with momentum: and buf) is 16-byte aligned at
//                  the tile's first element (with m % 4 == 0 every quad of the tile then): one
//                  workgroup-uniform test per tile; else 4-byte element accesses. A quad that
//                  crosses the tile's last column runs element by element. No access leaves rows
//                  [0, n) x columns [sbeg, send) of the tensor: every one is predicated on its own
//                  index.
//   record         psgd_sgd_hyper of the tile's tensor: six dwords read once per tile from
//                  workgroup-uniform addresses; the momentum, nesterov, first-step and weight-decay
//                  branches of sgd_update are scalar.
// The flat tail's update items (psgd_sgd_flat.cuh) lead the launch as workgroups blockIdx.x < nitems.
//
// LDS: 2 x 64 x (R + 4) floats = 34 816 / 67 584 bytes: two workgroups per CU at R = 128, which the
// register budget matches.
#include "psgd_sgd_flat.cuh"
#include "psgd_wide_sgd.cuh"  // sgd_epilogue over wide_pass (psgd_wide_pass.cuh)

namespace psgd {

template <int R, bool SHARED>
__global__ __launch_bounds__(kBlock, 2) void k_wide_apply_sgd(WideArgs a, WideSgdDst x) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 64 * (R + 4)];
    const int nf = x.flat.nitems;
    if (int(blockIdx.x) < nf) {  // workgroup-uniform
        flat_sgd_item<kBlock>(x.flat, x.y, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const int kq = int(threadIdx.x & 63) >> 4;
    const WideTile w = wide_tile(t, d);
    float* __restrict__ G = static_cast<float*>(a.grads[t.tensor]);
    const bool gvec = w.m % 4 == 0 && reinterpret_cast<uintptr_t>(G) % 16 == 0;

    f32x4_t acc[kSteps][4];
    if constexpr (SHARED) {
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[s][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        wide_pass<R, false>(acc, lds, a.res, a.nres, w);
    } else {
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[s][u] = ld_g4(G, w.n, w.m, w.o, w.sbeg + 64 * s + 16 * u + 4 * kq, w.send, gvec);
        wide_pass<R, true>(acc, lds, a.res, a.nres, w);  // reference powersgd.py:195-202
        if (w.ook) {
#pragma unroll
            for (int s = 0; s < kSteps; ++s)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t s4 = w.sbeg + 64 * s + 16 * u + fresh(4 * kq);
                    if (s4 < w.send) st_res4(G + w.o * w.m + s4, acc[s][u], s4, w.send, gvec);
                }
        }
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[s][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        wide_pass<R, false>(acc, lds, a.apx, a.nres, w);  // :211-219
    }
    if (!w.ook) return;  // past the last barrier
    // the tile's tensor: its record first, which says whether there is a buffer to look up at all
    const psgd_sgd_hyper h = x.y.hyper[d.tensor];
    float* __restrict__ P = static_cast<float*>(x.p[d.tensor]);
    if (h.momentum != 0.f)  // workgroup-uniform
        sgd_epilogue<SHARED, true>(acc, w, G, gvec, a.alpha, h, P, static_cast<float*>(x.y.bufs[d.tensor]));
    else
        sgd_epilogue<SHARED, false>(acc, w, G, gvec, a.alpha, h, P, nullptr);
}

namespace {

template <int R>
hipError_t wide_apply_sgd(const WideArgs& a, const WideSgdDst& x, int ntiles, hipStream_t s, int* waves) {
    const auto fn = a.shared ? &k_wide_apply_sgd<R, true> : &k_wide_apply_sgd<R, false>;
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    const int nb = ntiles + x.flat.nitems;
    if (nb == 0) return hipSuccess;
    timed_launch(fn, dim3(nb), dim3(kBlock), s, a, x);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_wide_apply_sgd(int R, const WideArgs& a, const WideSgdDst& x, int ntiles, hipStream_t s, int* waves) {
    switch (R) {
        case 64: return wide_apply_sgd<64>(a, x, ntiles, s, waves);
        case 128: return wide_apply_sgd<128>(a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace psgd
