// The final pass of psgd_aggregate_comm_dst_wide and psgd_aggregate_mixed_comm_dst_wide
// (psgd_onecall.cpp): effective ranks 33-128, the DDP hook's destination-table completions. Each
// tensor's average goes to the tensor's own destination (a view into a DDP bucket) at the element
// where k_wide_apply<float> would have stored it in the output slab.
//
//   k_wide_apply_dst<R, SHARED, BF16>   residual = G_0 - sum_k P_k Q_k^T (fp32, in place),
//                                       dst[tensor] = alpha sum_k Pbar_k Qbar_k^T   (fp32), or its
//                                       bf16 rounding to nearest even (BF16)
//
// Tile, accumulators, MFMA sequence and operand movement are k_wide_apply_mix's (wide_pass,
// psgd_wide_pass.cuh): the Q-side blocks staged once per workgroup in LDS (row stride R + 4 floats,
// two buffers, the next block's global loads ahead of the current MFMA chain, one barrier per
// block), the P side once per tile in registers. Every accumulator receives k_wide_apply<float>'s
// sequence, so the residual and the average acc x alpha (that kernel's one fp32 multiply; at world
// size 1 the sums themselves) have its bits: the step equals psgd_aggregate_comm into slabs followed
// by a copy (BF16: a rounding copy) bit for bit. SHARED (one rank): one accumulation, G read when the
// sums are complete, residual stored first, then the average. Else two passes with one accumulator
// set: from G_0 minus the local terms (the residual, stored), then from zero plus the all-reduced
// terms. Addresses are formed at use (fresh()), none lives across a pass.
//
// The epilogue. A lane owns, per column step, four row quads (u = 0 .. 3) of its row: columns
// sbeg + 64 step + 16 u + 4 kq .. + 3, stored at element o m + s4 of dst[MatDesc::tensor].
//   access width   chosen once per tile, workgroup-uniformly, from the destination alone (the
//                  residual's width is a test of its own, on G). fp32: 16 bytes where m % 4 == 0 and
//                  the destination is 16-byte aligned (with m % 4 == 0 every quad of the tensor then),
//                  else four 4-byte stores. bf16: one packed 8-byte store where m % 4 == 0 and the
//                  destination is 8-byte aligned, else four 2-byte stores. A quad that crosses the
//                  tile's last column runs element by element. Every store is predicated on its own
//                  row and column: nothing leaves rows [0, n) x columns [sbeg, send) of the tensor.
//   the average    pinned as a rounded value of its own before it is stored or rounded to bf16
//                  (avg_quad), so alpha x acc is never contracted into anything else.
//   cache policy   plain stores, as k_wide_apply<float>, k_wide_apply_mix and k_wide_apply_adam
//                  store: a wide plan's output pass has no nt / write-through instances (the plan's
//                  out_nt picks between instances of the rank buckets 1-32 only).
// The flat tail's items lead the launch as workgroups blockIdx.x < nitems: copy items
// (flat_copy_item, fp32) or round items (flat_round_item<kBlock, true>, bf16) from the plan's stage
// into the flat plan's own destinations.
//
// LDS: 2 x 64 x (R + 4) floats = 34 816 / 67 584 bytes: two workgroups per CU at R = 128, which the
// register budget matches (two waves per SIMD, no scratch: profiles/ddp_wide/resources.txt).
#include <type_traits>

#include "psgd_flat_copy.cuh"
#include "psgd_wide_pass.cuh"

namespace psgd {

namespace {

// One row quad of the average to its destination. `g` becomes a rounded value of its own first.
template <bool BF16>
__device__ __forceinline__ void avg_quad(std::conditional_t<BF16, bf16_t, float>* p, f32x4_t g, int64_t s4, int64_t send,
                                         bool vec) {
    asm volatile("" : "+v"(g));  // the average as k_wide_apply<float> stores it
    if constexpr (BF16) st_out4(p, g, s4, send, vec);
    else st_res4(p, g, s4, send, vec);
}

}  // namespace

template <int R, bool SHARED, bool BF16>
__global__ __launch_bounds__(kBlock, 2) void k_wide_apply_dst(WideArgs a, WideDst x) {
    using O = std::conditional_t<BF16, bf16_t, float>;
    __shared__ __attribute__((aligned(16))) float lds[2 * 64 * (R + 4)];
    const int nf = x.flat.nitems;
    if (int(blockIdx.x) < nf) {  // workgroup-uniform
        if constexpr (BF16) flat_round_item<kBlock, true>(x.flat, x.stage, blockIdx.x, x.unc_dst);
        else flat_copy_item<kBlock>(x.flat, x.stage, blockIdx.x, x.unc_dst);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const int kq = int(threadIdx.x & 63) >> 4;
    const WideTile w = wide_tile(t, d);
    float* __restrict__ G = static_cast<float*>(a.grads[t.tensor]);
    O* __restrict__ D = static_cast<O*>(x.dst[d.tensor]);
    const bool gvec = w.m % 4 == 0 && reinterpret_cast<uintptr_t>(G) % 16 == 0;
    // the tile's first element is (row 64 chunk, column sbeg): with m % 4 == 0 a multiple of four
    // elements from the tensor's base, so the base's alignment is the tile's
    const bool dvec = w.m % 4 == 0 && reinterpret_cast<uintptr_t>(D) % (4 * sizeof(O)) == 0;

    f32x4_t acc[kSteps][4];
    if constexpr (SHARED) {
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[s][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        wide_pass<R, false>(acc, lds, a.res, a.nres, w);
        if (!w.ook) return;  // past the last barrier
#pragma unroll
        for (int s = 0; s < kSteps; ++s) {
            if (s >= w.nsteps) continue;  // workgroup-uniform
            f32x4_t g[4];
            const int q4 = fresh(4 * kq);
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = ld_g4(G, w.n, w.m, w.o, w.sbeg + 64 * s + 16 * u + q4, w.send, gvec);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t s4 = w.sbeg + 64 * s + 16 * u + q4;
                if (s4 >= w.send) continue;
                st_res4(G + w.o * w.m + s4, g[u] - acc[s][u], s4, w.send, gvec);
                avg_quad<BF16>(D + w.o * w.m + s4, acc[s][u], s4, w.send, dvec);
            }
        }
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
        if (!w.ook) return;  // past the last barrier
        const float alpha = a.alpha;
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t s4 = w.sbeg + 64 * s + 16 * u + fresh(4 * kq);
                if (s4 < w.send) avg_quad<BF16>(D + w.o * w.m + s4, acc[s][u] * alpha, s4, w.send, dvec);
            }
    }
}

namespace {

template <int R, bool BF16>
hipError_t wide_apply_dst(const WideArgs& a, const WideDst& x, int ntiles, hipStream_t s, int* waves) {
    const auto fn = a.shared ? &k_wide_apply_dst<R, true, BF16> : &k_wide_apply_dst<R, false, BF16>;
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    const int nb = ntiles + x.flat.nitems;
    if (nb == 0) return hipSuccess;
    timed_launch(fn, dim3(nb), dim3(kBlock), s, a, x);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_wide_apply_dst(int R, bool bf16, const WideArgs& a, const WideDst& x, int ntiles, hipStream_t s,
                                 int* waves) {
    switch (R) {
        case 64: return bf16 ? wide_apply_dst<64, true>(a, x, ntiles, s, waves) : wide_apply_dst<64, false>(a, x, ntiles, s, waves);
        case 128: return bf16 ? wide_apply_dst<128, true>(a, x, ntiles, s, waves) : wide_apply_dst<128, false>(a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace psgd
