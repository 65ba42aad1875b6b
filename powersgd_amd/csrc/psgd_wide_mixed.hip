// The final pass of psgd_aggregate_mixed_wide[_comm] (psgd_mixed.cpp): effective ranks 33-128 on an
// fp32 error-feedback residual with the averages stored as bf16.
//
//   k_wide_apply_mix<R, SHARED>   residual = G_0 - sum_k P_k Q_k^T (fp32, in place),
//                                 output = bf16(alpha sum_k Pbar_k Qbar_k^T)
//
// The tile, the accumulator layout and the MFMA sequence of every accumulator are
// k_wide_apply<float>'s (psgd_wide.hip: 64 rows x kWideApplyCols columns per workgroup, 16 rows per
// wave, steps of kWideStep columns; terms ascending, 16-column blocks ascending, e ascending; the
// Q-side value negated on the A operand where the term is subtracted), so the fp32 residual and the
// fp32 values that are rounded are that kernel's bit for bit. What differs is where the operands
// come from:
//
//   Q side   the 64 rows of a column step of one term (64 x r fp32, contiguous in the panel) are
//            loaded ONCE per workgroup with 16-byte loads (ld_fac4: scalar where r % 4 != 0 or the
//            panel is not 16-byte aligned; zeros for columns >= r and rows past the tile) and
//            staged in LDS with a row stride of R + 4 floats. k_wide_apply loads them once per
//            wave. A wave's MFMA chain reads them back with one 16-byte LDS read per four MFMAs:
//            lane (ri, kq) reads row 16 u + ri, columns cc + 4 kq .. + 3. A 16-byte LDS read is
//            served 16 lanes at a time; the 16 ri lanes of one kq start at dword ri (R + 4) +
//            const, and (R + 4) mod 64 = 4 at R = 64 and 128, so their 16 x 4 dwords cover the 64
//            banks once. The staging stores of a row are contiguous.
//   staging  two buffers: the global loads of the next block (R / 16 quads per thread) are issued
//            before the current block's MFMA chain and stored to the other buffer after it; one
//            workgroup barrier per block. No other global load is issued while a block is in
//            flight (vmcnt retires in order: a later load would wait for the whole batch).
//   P side   a wave's own 16 rows of a term (R / 16 quads per lane) are loaded once per tile into
//            registers: the loops run terms outside, column steps inside (accumulators of
//            different steps are independent), with the accumulators of all four steps live.
//   G        SHARED (world size 1: one accumulation S, residual = G_0 - S, output = S): read when
//            the sums are complete. Otherwise the tile makes two passes over its terms with ONE
//            accumulator set: from G_0 minus the local terms (the residual, stored), then from
//            zero plus the all-reduced terms (the output); each accumulator still receives
//            k_wide_apply's sequence.
//
// LDS: 2 x 64 x (R + 4) floats = 34 816 / 67 584 bytes: two workgroups per CU at R = 128.
// The pass and its load / store helpers are psgd_wide_pass.cuh, shared with psgd_wide_adam.hip.
#include "psgd_wide_pass.cuh"

namespace psgd {

template <int R, bool SHARED>
__global__ __launch_bounds__(kBlock, 2) void k_wide_apply_mix(WideArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 64 * (R + 4)];
    const Tile t = a.tiles[blockIdx.x];
    const MatDesc d = a.mats[t.mat];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ri = lane & 15, kq = lane >> 4;
    WideTile w;
    w.n = d.n;
    w.m = d.m;
    w.poff = d.poff;
    w.qoff = d.qoff;
    w.r = d.r;
    const int64_t o0 = int64_t(t.chunk) * kWideOut + 16 * wave;
    w.active = o0 < w.n;
    w.o = o0 + ri;
    w.ook = w.o < w.n;
    w.sbeg = int64_t(t.strip) * kWideApplyCols;
    w.send = w.m < w.sbeg + kWideApplyCols ? w.m : w.sbeg + kWideApplyCols;
    w.nsteps = int((w.send - w.sbeg + kWideStep - 1) / kWideStep);
    float* __restrict__ G = static_cast<float*>(a.grads[t.tensor]);
    bf16_t* __restrict__ Out = static_cast<bf16_t*>(a.out) + d.out_off;
    const bool gvec = w.m % 4 == 0 && reinterpret_cast<uintptr_t>(G) % 16 == 0;
    const bool ovec = w.m % 4 == 0 && reinterpret_cast<uintptr_t>(Out) % 8 == 0;

    f32x4_t acc[kSteps][4];
    if constexpr (SHARED) {
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[s][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        wide_pass<R, false>(acc, lds, a.res, a.nres, w);
        if (!w.ook) return;
#pragma unroll
        for (int s = 0; s < kSteps; ++s) {
            f32x4_t g[4];
            const int q4 = fresh(4 * kq);
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = ld_g4(G, w.n, w.m, w.o, w.sbeg + 64 * s + 16 * u + q4, w.send, gvec);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t s4 = w.sbeg + 64 * s + 16 * u + q4;
                if (s4 >= w.send) continue;
                st_res4(G + w.o * w.m + s4, g[u] - acc[s][u], s4, w.send, gvec);
                st_out4(Out + w.o * w.m + s4, acc[s][u], s4, w.send, ovec);
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
        if (!w.ook) return;
        const float alpha = a.alpha;
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t s4 = w.sbeg + 64 * s + 16 * u + fresh(4 * kq);
                if (s4 < w.send) st_out4(Out + w.o * w.m + s4, acc[s][u] * alpha, s4, w.send, ovec);
            }
    }
}

namespace {

// `waves` (if non-null) receives the resident waves per SIMD of the instance that would run, 0
// when it uses scratch; no tiles: no launch
template <int R>
hipError_t wide_apply_mix(const WideArgs& a, int ntiles, hipStream_t s, int* waves) {
    const auto fn = a.shared ? &k_wide_apply_mix<R, true> : &k_wide_apply_mix<R, false>;
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    if (ntiles == 0) return hipSuccess;
    timed_launch(fn, dim3(ntiles), dim3(kBlock), s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_wide_apply_mix(int R, const WideArgs& a, int ntiles, hipStream_t s, int* waves) {
    switch (R) {
        case 64: return wide_apply_mix<64>(a, ntiles, s, waves);
        case 128: return wide_apply_mix<128>(a, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace psgd
