// What the LDS-staged final passes of a wide plan (effective ranks 33-128) share: k_wide_apply_mix
// (psgd_wide_mixed.hip) and k_wide_apply_adam (psgd_wide_adam.hip). The tile, the accumulator layout
// and the MFMA sequence of every accumulator are k_wide_apply<float>'s (psgd_wide.hip: 64 rows x
// kWideApplyCols columns per workgroup, 16 rows per wave, steps of kWideStep columns; terms
// ascending, 16-column blocks ascending, e ascending; the Q-side value negated on the A operand where
// the term is subtracted). psgd_wide_mixed.hip's header describes how the operands move.
#pragma once

#include "psgd_stream.cuh"

namespace psgd {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// F[row][c .. c + 3] of an [*, r] panel, zero past r or when !rowok (ld_fac4 of psgd_wide.hip)
__device__ __forceinline__ f32x4_t ld_fac4(const float* __restrict__ F, int64_t row, bool rowok, int c, int r, bool vec) {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (rowok && c < r) {
        const float* p = F + row * r + c;
        if (vec) {
            v = *reinterpret_cast<const f32x4_t*>(p);
        } else {
            v[0] = p[0];
            if (c + 1 < r) v[1] = p[1];
            if (c + 2 < r) v[2] = p[2];
            if (c + 3 < r) v[3] = p[3];
        }
    }
    return v;
}
__device__ __forceinline__ bool fac_vec(const float* F, int r) {
    return r % 4 == 0 && reinterpret_cast<uintptr_t>(F) % 16 == 0;
}

// four consecutive residual elements of row o from column s4, zero outside the matrix / past send
__device__ __forceinline__ f32x4_t ld_g4(const float* __restrict__ G, int64_t n, int64_t m, int64_t o, int64_t s4,
                                         int64_t send, bool vec) {
    f32x4_t g = {0.f, 0.f, 0.f, 0.f};
    if (o < n && s4 < send) {
        const float* p = G + o * m + s4;
        if (vec && s4 + 3 < send) {
            g = *reinterpret_cast<const f32x4_t*>(p);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (s4 + i < send) g[i] = p[i];
        }
    }
    return g;
}
__device__ __forceinline__ void st_res4(float* p, const f32x4_t& v, int64_t s4, int64_t send, bool vec) {
    if (vec && s4 + 3 < send) {
        *reinterpret_cast<f32x4_t*>(p) = v;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (s4 + i < send) p[i] = v[i];
    }
}
// a row quad of the output, rounded to nearest even: one 8-byte store, or four 2-byte stores
__device__ __forceinline__ void st_out4(bf16_t* p, const f32x4_t& v, int64_t s4, int64_t send, bool vec) {
    if (vec && s4 + 3 < send) {
        const v2u x = {uint32_t(f2bf(v[0])) | (uint32_t(f2bf(v[1])) << 16), uint32_t(f2bf(v[2])) | (uint32_t(f2bf(v[3])) << 16)};
        *reinterpret_cast<v2u*>(p) = x;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (s4 + i < send) p[i] = f2bf(v[i]);
    }
}

// A value the compiler recomputes addresses from: an epilogue's sixteen row-quad addresses are then
// formed where they are used instead of being kept in registers across a pass (32 VGPRs)
__device__ __forceinline__ int fresh(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

constexpr int kSteps = kWideApplyCols / kWideStep;  // column steps of a tile
static_assert(kSteps == 4 && kWideOut == 64 && kBlock == 256, "k_wide_apply_mix: four waves x 16 rows, four steps");

// What a pass needs of its tile
struct WideTile {
    int64_t n, m, poff, qoff;
    int64_t o, sbeg, send;  // the lane's row; the tile's columns [sbeg, send)
    int r, nsteps;          // steps with columns: 1 .. kSteps (workgroup-uniform)
    bool active, ook;       // the wave has rows of the matrix; the lane's row is one
};

// the tile of workgroup (t, d) as the lane sees it
__device__ __forceinline__ WideTile wide_tile(const Tile& t, const MatDesc& d) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ri = lane & 15;
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
    return w;
}

// One pass over the terms (P_k, Q_k), k < nterms: acc[step][u] += sign P_k Q_k^T on the four
// 16 x 16 sub-tiles u of each step. Blocks in (term, step) order through the two LDS buffers.
template <int R, bool NEG>
__device__ __forceinline__ void wide_pass(f32x4_t (&acc)[kSteps][4], float* __restrict__ lds, const Terms& T, int nterms,
                                          const WideTile& w) {
    constexpr int LD = R + 4;      // padded row stride (floats)
    constexpr int NQ = R / 16;     // staged quads per thread: 64 rows x R / 4 quads over 256 threads
    constexpr int QPR = R / 4;     // quads per staged row
    const int tid = threadIdx.x, lane = tid & 63, ri = lane & 15, kq = lane >> 4;
    const int r = w.r;
    f32x4_t pre[NQ];
    auto load_block = [&](int k, int step) {
        const float* __restrict__ Q = T.q[k] + w.qoff;
        const bool vq = fac_vec(Q, r);
        const int64_t s0 = w.sbeg + int64_t(step) * kWideStep;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int idx = tid + kBlock * j, row = idx / QPR, c = 4 * (idx % QPR);
            pre[j] = ld_fac4(Q, s0 + row, s0 + row < w.send, c, r, vq);
        }
    };
    auto store_block = [&](float* buf) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int idx = tid + kBlock * j, row = idx / QPR, c = 4 * (idx % QPR);
            *reinterpret_cast<f32x4_t*>(buf + row * LD + c) = pre[j];
        }
    };
    __syncthreads();  // every wave is done with both buffers (the pass before this one)
    if (nterms <= 0) return;
    load_block(0, 0);
    store_block(lds);
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < nterms; ++k) {
        const float* __restrict__ P = T.p[k] + w.poff;
        const bool vp = fac_vec(P, r);
        f32x4_t pf[NQ];
#pragma unroll
        for (int b = 0; b < NQ; ++b) pf[b] = ld_fac4(P, w.o, w.ook && 16 * b < r, 16 * b + 4 * kq, r, vp);
#pragma unroll
        for (int step = 0; step < kSteps; ++step) {
            if (step >= w.nsteps) continue;  // workgroup-uniform
            const bool wrap = step + 1 == w.nsteps;
            const bool more = !wrap || k + 1 < nterms;  // workgroup-uniform
            if (more) load_block(wrap ? k + 1 : k, wrap ? 0 : step + 1);
            if (w.active) {  // wave-uniform
                const float* __restrict__ buf = lds + cur * (64 * LD);
#pragma unroll
                for (int b = 0; b < NQ; ++b) {
                    if (16 * b < r) {  // wave-uniform
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const f32x4_t fs = *reinterpret_cast<const f32x4_t*>(buf + (16 * u + ri) * LD + 16 * b + 4 * kq);
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[step][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(NEG ? -fs[e] : fs[e], pf[b][e],
                                                                                  acc[step][u], 0, 0, 0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);  // keep the LDS reads of later blocks out of this one's registers
                }
            }
            if (more) store_block(lds + (cur ^ 1) * (64 * LD));
            __syncthreads();
            cur ^= 1;
        }
    }
}

}  // namespace psgd
