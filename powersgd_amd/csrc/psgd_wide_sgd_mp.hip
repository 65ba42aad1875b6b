// The final pass of psgd_aggregate_mixed_comm_sgd_wide (psgd_onecall.cpp): effective ranks 33-128, the
// master-weight form of k_wide_apply_sgd (psgd_wide_sgd.hip, whose header describes the tile, the
// pass and the epilogue's two bodies, ring depths and access widths; sgd_epilogue is shared through
// psgd_wide_sgd.cuh).
//
//   k_wide_apply_sgd_mp<R, SHARED>  residual = G_0 - sum_k P_k Q_k^T (the fp32 residual of bf16
//                                   gradients, in place), g = alpha sum_k Pbar_k Qbar_k^T, never
//                                   stored: (p, buf) <- THE UPDATE(g, p, buf) on the fp32 master
//                                   weight, w = bf16(p') at the bf16 model tensor
//
// w is store only: the quad of p' the lane has just stored is rounded to nearest even and leaves as
// one 8-byte store where m % 4 == 0 and the model tensor is 8-byte aligned (a test of its own, once
// per tile), else in 2-byte pieces; like every access of the epilogue it is predicated on its own
// row and column. It adds no quad to the ring: the register and LDS budgets are k_wide_apply_sgd's
// (profiles/sgd_master/resources.txt). A unit of its own, so k_wide_apply_sgd's unit compiles as before.
#include "psgd_sgd_flat.cuh"  // flat_sgd_mp_item: the flat tail's update items
#include "psgd_wide_sgd.cuh"

namespace psgd {

// The master-weight form (psgd_aggregate_mixed_comm_sgd_wide): the same pass on the fp32 residual of
// bf16 gradients, the update on the fp32 master weights, and bf16(p') stored at the model tensors.
// The separate body without a buffer operand stays: a tile whose momentum is 0 moves p and w alone.
template <int R, bool SHARED>
__global__ __launch_bounds__(kBlock, 2) void k_wide_apply_sgd_mp(WideArgs a, WideSgdMpDst x) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 64 * (R + 4)];
    const int nf = x.flat.nitems;
    if (int(blockIdx.x) < nf) {  // workgroup-uniform
        flat_sgd_mp_item<kBlock>(x.flat, x.y, blockIdx.x);
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
    const psgd_sgd_hyper h = x.y.x.hyper[d.tensor];
    float* __restrict__ P = static_cast<float*>(x.p[d.tensor]);
    bf16_t* __restrict__ W = static_cast<bf16_t*>(x.y.ws[d.tensor]);
    if (h.momentum != 0.f)  // workgroup-uniform
        sgd_epilogue<SHARED, true, true>(acc, w, G, gvec, a.alpha, h, P, static_cast<float*>(x.y.x.bufs[d.tensor]), W);
    else
        sgd_epilogue<SHARED, false, true>(acc, w, G, gvec, a.alpha, h, P, nullptr, W);
}

namespace {

template <int R>
hipError_t wide_apply_sgd_mp(const WideArgs& a, const WideSgdMpDst& x, int ntiles, hipStream_t s, int* waves) {
    const auto fn = a.shared ? &k_wide_apply_sgd_mp<R, true> : &k_wide_apply_sgd_mp<R, false>;
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    const int nb = ntiles + x.flat.nitems;
    if (nb == 0) return hipSuccess;
    timed_launch(fn, dim3(nb), dim3(kBlock), s, a, x);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_wide_apply_sgd_mp(int R, const WideArgs& a, const WideSgdMpDst& x, int ntiles, hipStream_t s,
                                    int* waves) {
    switch (R) {
        case 64: return wide_apply_sgd_mp<64>(a, x, ntiles, s, waves);
        case 128: return wide_apply_sgd_mp<128>(a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace psgd
