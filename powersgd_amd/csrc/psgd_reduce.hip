// Deterministic reduction of the product partials (k_reduce).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "psgd_internal.h"
#include "psgd_stream.cuh"
#include "psgd_chain.cuh"  // wave_allsum_f64

namespace psgd {

// Sums the partials of each factor element in a FIXED order (the even product's segments down
// a column strip, the odd product's column strips): bitwise reproducible, no atomics.

// One item = up to 64 * per consecutive elements of one factor (per = 4, or 1 for factors with
// many partials: RedItem::per) with one partial layout (RedItem::pbase / pstride / np).
// per = 4: one 16-byte load per partial when the item's partial runs are 16-byte aligned (lane
// l owns elements 4l .. 4l+3), else four 256-byte wave loads (lane l owns l, l+64, l+128,
// l+192). Wave w adds the partials [w*np/4, (w+1)*np/4) of each element in order, then wave 0
// adds the four wave sums in order: every element is summed in the same fixed order on every
// run, whatever the layout.
#ifndef PSGD_RED_SHORT
#define PSGD_RED_SHORT 8
#endif
__device__ __forceinline__ int red_elem(bool vec, int lane, int j) { return vec ? 4 * lane + j : lane + 64 * j; }

__global__ __launch_bounds__(kBlock) void k_reduce(ReduceArgs a) {
    __shared__ float red[kWaves * kRedItem];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (int(blockIdx.x) >= a.nmain) {  // fused normalisation of the in-factor (rank 1)
        if (wave != 0) return;
        const RedItem it = a.nitems[blockIdx.x - a.nmain];
        const MatDesc d = a.mats[it.mat];
        const int64_t base = (a.even ? d.poff : d.qoff) + it.start;
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // in flight together with the norm's loads
            const int e = red_elem(false, lane, j);
            x[j] = a.raw[base + (e < it.cnt ? e : 0)];
        }
        const float dn = group_norm_ss(a.ss_in, a.grng_in, d.group);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = red_elem(false, lane, j);
            if (j < it.per && e < it.cnt) {
                const float v = x[j] / dn;  // matrix.div_(max(norm, eps))
                a.xstate[base + e] = v;
                a.hx[base + e] = v;
            }
        }
        return;
    }
    const RedItem it = a.items[blockIdx.x];
    const MatDesc d = a.mats[it.mat];
    const int per = it.per, cnt = it.cnt;
    const int64_t ps = it.pstride;
    const bool vec = per == 4 && ((it.pbase | ps | int64_t(cnt)) & 3) == 0;  // uniform per workgroup
    const int np = it.np;
    const int c0 = wave * np / kWaves, c1 = (wave + 1) * np / kWaves;
    // wave 0's first group-norm loads go out before the partials' (group_norm_ss's order:
    // lane-strided sums from 0, then the wave tree), so the two round trips overlap
    const bool nrm = a.ss_in != nullptr && wave == 0;
    int gb = 0, ge = 0;
    float ssv = 0.f;
    if (nrm) {
        gb = a.grng_in[2 * d.group];
        ge = a.grng_in[2 * d.group + 1];
        ssv = gb + lane < ge ? a.ss_in[gb + lane] : 0.f;
    }
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    // loads issued 16 at a time (clamped, unconditional): the partials were just written on
    // other XCDs, so each batch is one MALL round trip
    const gptr<const float> pb = gconst<float>(a.part) + it.pbase;
    if (vec) {
        const int e0 = red_elem(true, lane, 0);
        const gptr<const float> p = pb + (e0 < cnt ? e0 : 0);
        // batches of kB partials; a wave with at most PSGD_RED_SHORT partials issues only that
        // many loads (no clamped repeats): k_reduce 6.2 -> 5.5-5.7 us on cfg3,
        // cfg3 / cfg2 steps 0.0910 / 0.0757-0.0760 -> 0.0905-0.0907 / 0.0754-0.0756 ms
        // (profiles/r05/reduce)
        auto run = [&](auto KB) {
            constexpr int kB = decltype(KB)::value;
            for (int c = c0; c < c1; c += kB) {
                float v[kB][4];
#pragma unroll
                for (int q = 0; q < kB; ++q) {
                    const v4f x = *(gptr<const v4f>)(p + int64_t(c + q < c1 ? c + q : c0) * ps);
                    v[q][0] = x.x; v[q][1] = x.y; v[q][2] = x.z; v[q][3] = x.w;
                }
#pragma unroll
                for (int q = 0; q < kB; ++q)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        keep(v[q][j]);
                        s[j] += c + q < c1 ? v[q][j] : 0.f;
                    }
            }
        };
        if (PSGD_RED_SHORT > 0 && c1 - c0 <= PSGD_RED_SHORT)
            run(std::integral_constant<int, (PSGD_RED_SHORT > 0 ? PSGD_RED_SHORT : 1)>{});
        else
            run(std::integral_constant<int, 16>{});
    } else if (per == 4) {
        int ec[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = red_elem(false, lane, j);
            ec[j] = e < cnt ? e : 0;
        }
        constexpr int kB = 4;
        for (int c = c0; c < c1; c += kB) {
            float v[kB][4];
#pragma unroll
            for (int q = 0; q < kB; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[q][j] = pb[int64_t(c + q < c1 ? c + q : c0) * ps + ec[j]];
#pragma unroll
            for (int q = 0; q < kB; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    keep(v[q][j]);
                    s[j] += c + q < c1 ? v[q][j] : 0.f;
                }
        }
    } else {
        // many partials per element (np > kRedWide, e.g. the odd-even pass's row blocks): 32 of
        // a wave's partials in flight at once (two round trips where 16 took four on 256
        // partials; the sum order is the same)
        const gptr<const float> p = pb + (lane < cnt ? lane : 0);
        constexpr int kB = 32;
        for (int c = c0; c < c1; c += kB) {
            float v[kB];
#pragma unroll
            for (int q = 0; q < kB; ++q) v[q] = p[int64_t(c + q < c1 ? c + q : c0) * ps];
#pragma unroll
            for (int q = 0; q < kB; ++q) {
                keep(v[q]);
                s[0] += c + q < c1 ? v[q] : 0.f;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < per) red[wave * kRedItem + j * 64 + lane] = s[j];
    __syncthreads();
    if (wave != 0) return;
    float nv = 1.f;
    if (nrm) {
        for (int i = gb + lane + 64; i < ge; i += 64) ssv += a.ss_in[i];
        nv = sqrtf(wave_allsum(ssv));
        nv = nv > 1e-16f ? nv : 1e-16f;
    }
    const int64_t dbase = (a.even ? d.qoff : d.poff) + it.start;
    float sq = 0.f;
    float tv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        tv[j] = 0.f;
        if (j >= per) continue;
        const int o = j * 64 + lane;
        float t = ((red[o] + red[kRedItem + o]) + red[2 * kRedItem + o]) + red[3 * kRedItem + o];
        if (nrm) t = t / nv;  // G^T (x / d) == (G^T x) / d up to rounding
        const int e = red_elem(vec, lane, j);
        if (e < cnt) {
            a.yloc[dbase + e] = t;
            a.state[dbase + e] = t;
            if (a.xout) st_slot(a.xout + dbase + e, t);
            sq = fmaf(t, t, sq);
            tv[j] = t;
        }
    }
    if (a.ss_out) {  // this output is the next iteration's in-factor: its sum of squares
        const float v = wave_allsum(sq);
        if (lane == 0) a.ss_out[blockIdx.x] = v;
    }
    if (a.gram) {
        // folded orthonormalisation: the upper Gram of this item's rows (r in {2, 4}; items
        // start on a row and hold whole rows). The outputs go to LDS in element order (wave 0
        // alone: its own earlier reads of `red` are ordered before these writes), then lane l
        // takes rows l, l + 64, ...; fp64 products and sums, one fixed-order wave tree per entry.
        const int r = a.gram_r, ng = r * (r + 1) / 2;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < per) red[vec ? 4 * lane + j : lane + 64 * j] = tv[j];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int nrow = 64 * per / r;
        double g[kGramStride];
#pragma unroll
        for (int e = 0; e < kGramStride; ++e) g[e] = 0.0;
        auto rows = [&](auto RT) {  // compile-time r: register-indexed Gram entries
            constexpr int RC = decltype(RT)::value;
            for (int row = lane; row < nrow; row += 64) {
                float x[RC];
#pragma unroll
                for (int c = 0; c < RC; ++c) x[c] = red[row * RC + c];
                int e = 0;
#pragma unroll
                for (int c = 0; c < RC; ++c)
#pragma unroll
                    for (int b = c; b < RC; ++b) g[e++] += double(x[c]) * double(x[b]);
            }
        };
        if (r == 4)
            rows(std::integral_constant<int, 4>{});
        else
            rows(std::integral_constant<int, 2>{});
#pragma unroll
        for (int e = 0; e < kGramStride; ++e) {
            if (e < ng) {
                const double t = wave_allsum_f64(g[e]);
                if (lane == 0) a.gram[int64_t(blockIdx.x) * kGramStride + e] = t;
            }
        }
    }
}

hipError_t launch_reduce(const ReduceArgs& a, int nitems, hipStream_t s) {
    k_reduce<<<nitems, kBlock, 0, s>>>(a);  // nitems = nmain + nnorm
    return hipGetLastError();
}

}  // namespace psgd
