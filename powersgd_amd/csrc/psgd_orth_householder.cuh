// Householder orthonormalisation kernels (k_orth, k_orth_reg, k_orth_wy), the paper-code
// Gram-Schmidt variant (k_orth_mgs), the selection among them and their instance tables.
// Included by psgd_orth.hip only.
#pragma once

#include "psgd_chain.cuh"

namespace psgd {

// Diagnostic-only phase stamps of the orthonormalisation kernels (tools/orth_stamps.hip and
// tools/chol_stamps.hip build psgd_orth.hip with PSGD_STAMPS; the library build never
// executes a stamp).
#ifdef PSGD_STAMPS
__device__ unsigned long long g_stamps[64];
#define PSGD_STAMP(i)                                                                         \
    do {                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        unsigned long long t_;                                                                \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");           \
        if (threadIdx.x == 0 && blockIdx.x == 0) g_stamps[i] = t_;                            \
        __builtin_amdgcn_sched_barrier(0);                                                    \
    } while (0)
#else
#define PSGD_STAMP(i) \
    do {              \
    } while (0)
#endif

// Sum NV floats over a workgroup of NW waves; result in every thread. `red` holds
// 2 * NW * SLOT floats (double-buffered by `phase`, so one barrier per call suffices).
// SLOT is the largest NV the kernel sums: the two buffers sit at fixed offsets, so calls
// of different widths never overlap the buffer the previous call is still being read from.
template <int NV, int NW, int SLOT>
__device__ __forceinline__ void wg_sum(float (&v)[NV], float* red, int& phase) {
    static_assert(NV <= SLOT, "wg_sum: NV exceeds the buffer slot");
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_allsum(v[i]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* buf = red + phase * NW * SLOT;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) buf[wave * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float s = buf[i];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += buf[w * NV + i];
        v[i] = s;
    }
    phase ^= 1;
}

// ---------------------------------------------------------------- orthonormalise
// reference powersgd/orthogonalization.py:4-8.
//   rank 1 : x /= max(||x||_F over the WHOLE shape group, 1e-16)
//   rank>1 : x = Q of the Householder QR of each [k, r] panel — LAPACK geqr2 + org2r
//            conventions (beta = -sign(alpha)*||col||, tau = 0 for an all-zero column,
//            so a zero panel yields the leading identity columns, as torch.linalg.qr does).
// The panel is staged in LDS when it fits, else worked on in place in the history buffer.
template <int R>
__global__ __launch_bounds__(kBlock) void k_orth(OrthArgs a, int64_t lds_floats) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double redd[kWaves];
    __shared__ float red[kWaves * (R > 1 ? R : 1)];
    __shared__ float tau[(R + 3) / 4 * 4];  // keep the static LDS a multiple of 16 bytes
    const OrthUnit u = a.units[blockIdx.x];
    float* st = a.state + u.off;
    float* hx = a.hx + u.off;
    const int64_t total = u.k * u.r * u.count;
    const int tid = threadIdx.x;
    if (a.save) {
        float* sv = a.save + u.off;
        for (int64_t i = tid; i < total; i += kBlock) sv[i] = st[i];
    }
    if (u.r == 1) {
        double s[1] = {0.0};
        for (int64_t i = tid; i < total; i += kBlock) {
            const double x = st[i];
            s[0] += x * x;
        }
        block_sum_nw<double, 1, kWaves>(s, redd);
        const float nrm = float(sqrt(s[0]));
        const float d = nrm > 1e-16f ? nrm : 1e-16f;  // torch.maximum(norm, eps)
        for (int64_t i = tid; i < total; i += kBlock) {
            const float x = st[i] / d;
            st[i] = x;
            hx[i] = x;
        }
        return;
    }
    if constexpr (R > 1) {
        const bool in_lds = total <= lds_floats;
        float* A = in_lds ? smem : hx;
        for (int64_t i = tid; i < total; i += kBlock) A[i] = st[i];
        __syncthreads();
        householder_q<R>(A, u.k, u.r, red, tau);
        for (int64_t i = tid; i < total; i += kBlock) {
            const float x = A[i];
            st[i] = x;
            if (in_lds) hx[i] = x;
        }
    }
}

// ----------------------------------------------------------- fast orthonormalise
constexpr int kOrthThreads = 1024;
constexpr int kOrthWaves = kOrthThreads / 64;

// rank 1: x /= max(||x||, 1e-16) over the whole shape group (two streaming passes, the
// second one from L2). Optionally saves the pre-normalisation values.
template <int NT = kOrthThreads>
__device__ void orth_joint_norm(const OrthArgs& a, const OrthUnit& u, double* rd) {
    float* __restrict__ st = a.state + u.off;
    float* __restrict__ hx = a.hx + u.off;
    float* __restrict__ sv = a.save ? a.save + u.off : nullptr;
    const int64_t total = u.k * u.count;
    const int tid = threadIdx.x;
    constexpr int U = 8;
    float part = 0.f;
    // a group of at most U1 * NT values (every rank-1 group of cfg2 at W > 1): all loads in
    // one round trip, no second pass; the per-thread order of the sums is the batched loop's
    constexpr int U1 = 16;
    if (total <= int64_t(U1) * NT) {
        float x[U1];
#pragma unroll
        for (int q = 0; q < U1; ++q) {  // unconditional loads from clamped indices (no branches)
            const int64_t i = tid + int64_t(q) * NT;
            x[q] = st[i < total ? i : 0];
        }
#pragma unroll
        for (int q = 0; q < U1; ++q) {
            const int64_t i = tid + int64_t(q) * NT;
            keep(x[q]);
            x[q] = i < total ? x[q] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < U1; ++q) part = fmaf(x[q], x[q], part);
        double s = wave_allsum(part);
        if ((tid & 63) == 0) rd[tid >> 6] = s;
        __syncthreads();
        s = 0.0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) s += rd[w];
        const float nrm = float(sqrt(s));
        const float d = nrm > 1e-16f ? nrm : 1e-16f;
        if (a.rfac)
            for (int c = tid; c < u.count; c += NT) a.rfac[u.off + int64_t(c) * u.k] = d;
#pragma unroll
        for (int q = 0; q < U1; ++q) {
            const int64_t i = tid + int64_t(q) * NT;
            if (i < total) {
                if (sv) sv[i] = x[q];
                const float y = x[q] / d;
                st[i] = y;
                hx[i] = y;
            }
        }
        return;
    }
    for (int64_t base = tid; base < total; base += int64_t(U) * NT) {
        float x[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {  // unconditional loads from clamped indices (no branches)
            const int64_t i = base + int64_t(q) * NT;
            x[q] = st[i < total ? i : 0];
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t i = base + int64_t(q) * NT;
            keep(x[q]);
            x[q] = i < total ? x[q] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < U; ++q) part = fmaf(x[q], x[q], part);
    }
    // block sum in double (wave partials in fp32 are exact enough: <= 64 * U terms each)
    double s = wave_allsum(part);
    if ((tid & 63) == 0) rd[tid >> 6] = s;
    __syncthreads();
    s = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += rd[w];
    const float nrm = float(sqrt(s));
    const float d = nrm > 1e-16f ? nrm : 1e-16f;  // torch.maximum(norm, eps)
    if (a.rfac)  // x = (x / d) d: R' = d for every panel of the group
        for (int c = tid; c < u.count; c += NT) a.rfac[u.off + int64_t(c) * u.k] = d;
    for (int64_t base = tid; base < total; base += int64_t(U) * NT) {
        float x[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t i = base + int64_t(q) * NT;
            x[q] = st[i < total ? i : 0];
        }
#pragma unroll
        for (int q = 0; q < U; ++q) keep(x[q]);
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t i = base + int64_t(q) * NT;
            if (i < total) {
                if (sv) sv[i] = x[q];
                const float y = x[q] / d;
                st[i] = y;
                hx[i] = y;
            }
        }
    }
}

// rank > 1: the k x r panel lives in registers (thread t owns rows t + 1024 q, q < RPT);
// LAPACK geqr2 + org2r as 3r - 1 workgroup reductions.
template <int R, int RPT>
__global__ __launch_bounds__(kOrthThreads) void k_orth_reg(OrthArgs a) {
    constexpr int kSlot = R > 2 ? R : 2;  // widest wg_sum below
    __shared__ __attribute__((aligned(16))) float red[2 * kOrthWaves * kSlot];
    const OrthUnit u = a.units[blockIdx.x];
    if (u.r == 1) {
        orth_joint_norm(a, u, reinterpret_cast<double*>(red));
        return;
    }
    if constexpr (R > 1) {
        PSGD_STAMP(0);
        const int r = u.r;
        const int64_t k = u.k;
        const int tid = threadIdx.x;
        float* __restrict__ st = a.state + u.off;
        float* __restrict__ sv = a.save ? a.save + u.off : nullptr;
        float A[RPT][R];
        // every load first (all in flight together), then the save-copy stores
#pragma unroll
        for (int q = 0; q < RPT; ++q) {  // unconditional loads from clamped indices (no branches)
            const int64_t i = tid + int64_t(q) * kOrthThreads;
            const int64_t ic = i < k ? i : 0;
#pragma unroll
            for (int c = 0; c < R; ++c) A[q][c] = st[ic * r + (c < r ? c : 0)];
        }
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int64_t i = tid + int64_t(q) * kOrthThreads;
#pragma unroll
            for (int c = 0; c < R; ++c) {
                keep(A[q][c]);
                A[q][c] = (i < k && c < r) ? A[q][c] : 0.f;
            }
        }
        if (sv) {
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                const int64_t i = tid + int64_t(q) * kOrthThreads;
                if (i < k) {
#pragma unroll
                    for (int c = 0; c < R; ++c)
                        if (c < r) sv[i * r + c] = A[q][c];
                }
            }
        }
        PSGD_STAMP(1);
        int phase = 0;
        float tau[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            tau[j] = 0.f;
            if (j >= r) continue;
            PSGD_STAMP(2 + 2 * j);
            float v2[2] = {0.f, 0.f};  // sum_{i>j} A[i][j]^2, alpha = A[j][j]
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                const int64_t i = tid + int64_t(q) * kOrthThreads;
                const float x = A[q][j];
                if (i > j && i < k) v2[0] = fmaf(x, x, v2[0]);
                if (i == j) v2[1] = x;
            }
            wg_sum<2, kOrthWaves, kSlot>(v2, red, phase);
            PSGD_STAMP(3 + 2 * j);
            const float alpha = v2[1];
            float tj = 0.f;
            if (v2[0] != 0.f) {
                const float beta = -copysignf(hypotf(alpha, sqrtf(v2[0])), alpha);
                tj = (beta - alpha) / beta;
                const float scal = 1.f / (alpha - beta);
#pragma unroll
                for (int q = 0; q < RPT; ++q) {
                    const int64_t i = tid + int64_t(q) * kOrthThreads;
                    if (i > j && i < k) A[q][j] *= scal;
                    if (i == j) A[q][j] = beta;
                }
            }
            tau[j] = tj;
            if (tj != 0.f && j + 1 < r) {  // apply H_j to A[j:, j+1:]
                float w[R];
#pragma unroll
                for (int c = 0; c < R; ++c) w[c] = 0.f;
#pragma unroll
                for (int q = 0; q < RPT; ++q) {
                    const int64_t i = tid + int64_t(q) * kOrthThreads;
                    const float vi = i == j ? 1.f : ((i > j && i < k) ? A[q][j] : 0.f);
#pragma unroll
                    for (int c = j + 1; c < R; ++c) w[c] = fmaf(vi, A[q][c], w[c]);
                }
                wg_sum<R, kOrthWaves, kSlot>(w, red, phase);
#pragma unroll
                for (int q = 0; q < RPT; ++q) {
                    const int64_t i = tid + int64_t(q) * kOrthThreads;
                    const float vi = i == j ? 1.f : ((i > j && i < k) ? A[q][j] : 0.f);
#pragma unroll
                    for (int c = j + 1; c < R; ++c) A[q][c] -= tj * vi * w[c];
                }
            }
        }
        PSGD_STAMP(40);
        // org2r: Q = H_0 ... H_{r-1} I[:, :r]
#pragma unroll
        for (int j = R - 1; j >= 0; --j) {
            if (j >= r) continue;
            const float tj = tau[j];
            if (j + 1 < r && tj != 0.f) {
                float w[R];
#pragma unroll
                for (int c = 0; c < R; ++c) w[c] = 0.f;
#pragma unroll
                for (int q = 0; q < RPT; ++q) {
                    const int64_t i = tid + int64_t(q) * kOrthThreads;
                    const float vi = i == j ? 1.f : ((i > j && i < k) ? A[q][j] : 0.f);
#pragma unroll
                    for (int c = j + 1; c < R; ++c) w[c] = fmaf(vi, A[q][c], w[c]);
                }
                wg_sum<R, kOrthWaves, kSlot>(w, red, phase);
#pragma unroll
                for (int q = 0; q < RPT; ++q) {
                    const int64_t i = tid + int64_t(q) * kOrthThreads;
                    const float vi = i == j ? 1.f : ((i > j && i < k) ? A[q][j] : 0.f);
#pragma unroll
                    for (int c = j + 1; c < R; ++c) A[q][c] -= tj * vi * w[c];
                }
            }
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                const int64_t i = tid + int64_t(q) * kOrthThreads;
                if (i > j && i < k) A[q][j] *= -tj;
                else if (i == j) A[q][j] = 1.f - tj;
                else if (i < j) A[q][j] = 0.f;
            }
        }
        PSGD_STAMP(41);
        float* __restrict__ hx = a.hx + u.off;
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int64_t i = tid + int64_t(q) * kOrthThreads;
            if (i < k) {
#pragma unroll
                for (int c = 0; c < R; ++c)
                    if (c < r) {
                        st[i * r + c] = A[q][c];
                        hx[i * r + c] = A[q][c];
                    }
            }
        }
        PSGD_STAMP(42);
    }
}

// ------------------------------------------------- WY-form Householder (fast path) ----
// LAPACK geqr2 + org2r semantics with two latency cuts (stamps: each workgroup reduction
// costs ~1k cycles, the arithmetic is negligible):
//  * per column j ONE reduction gathers ||A[j+1:, j]||^2, alpha = A[j][j], the dots
//    d_c = A[j+1:, j] . A[j+1:, c] and A[j][c] (c > j): w_c = A[j][c] + scal * d_c is the
//    same quantity as LAPACK's slarf w = v^T C with v = [1; scal * A[j+1:, j]];
//  * Q = H_0 ... H_{r-1} [I; 0] = [I; 0] - V T V1^T (compact WY, LAPACK slarft: T upper
//    triangular from tau and V^T V), i.e. ONE more reduction instead of r - 1 in org2r.
// NW = waves per panel: NW = 1 -> one wave per panel (4 panels per 256-thread workgroup,
// no barriers); NW = 4/8/16 -> the whole workgroup of 64*NW threads works on one panel
// (rows tid + 64*NW*q, cross-wave sums through LDS). More waves per panel means fewer rows
// per wave and several waves per SIMD to hide each other's latency.
template <int NV, int NW, int SLOT>
__device__ __forceinline__ void grp_sum(float (&v)[NV], float* red, int& phase) {
    static_assert(NV <= SLOT, "grp_sum: NV exceeds the buffer slot");
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_allsum(v[i]);
    if constexpr (NW > 1) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        float* buf = red + phase * (NW + 1) * SLOT;
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) buf[wave * NV + i] = v[i];
        }
        __syncthreads();
        if constexpr (NW * NV <= 64) {  // few partials: every thread adds them itself
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                float sum = buf[i];
#pragma unroll
                for (int w = 1; w < NW; ++w) sum += buf[w * NV + i];
                v[i] = sum;
            }
        } else {  // thread i adds partial i over the waves (same order), then all read
            if (threadIdx.x < NV) {
                float sum = buf[threadIdx.x];
#pragma unroll
                for (int w = 1; w < NW; ++w) sum += buf[w * NV + threadIdx.x];
                buf[NW * NV + threadIdx.x] = sum;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = buf[NW * NV + i];
        }
        phase ^= 1;
    }
}

// rank-1 unit handled by the NW waves of its panel group
template <int NW>
__device__ void joint_norm_grp(const OrthArgs& a, const OrthUnit& u, float* red) {
    constexpr int NT = 64 * NW;
    const int t = NW == 1 ? (threadIdx.x & 63) : threadIdx.x;
    float* __restrict__ st = a.state + u.off;
    float* __restrict__ hx = a.hx + u.off;
    float* __restrict__ sv = a.save ? a.save + u.off : nullptr;
    const int64_t total = u.k * u.count;
    constexpr int U = 8;
    float part[1] = {0.f};
    for (int64_t base = t; base < total; base += int64_t(U) * NT) {
        float x[U];
#pragma unroll
        for (int q = 0; q < U; ++q) x[q] = st[base + q * NT < total ? base + q * NT : 0];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            keep(x[q]);
            part[0] = fmaf(base + q * NT < total ? x[q] : 0.f, base + q * NT < total ? x[q] : 0.f, part[0]);
        }
    }
    int phase = 0;
    grp_sum<1, NW, 1>(part, red, phase);
    const float nrm = sqrtf(part[0]);
    const float d = nrm > 1e-16f ? nrm : 1e-16f;  // torch.maximum(norm, eps)
    for (int64_t base = t; base < total; base += int64_t(U) * NT) {
        float x[U];
#pragma unroll
        for (int q = 0; q < U; ++q) x[q] = st[base + q * NT < total ? base + q * NT : 0];
#pragma unroll
        for (int q = 0; q < U; ++q) keep(x[q]);
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t i = base + q * NT;
            if (i < total) {
                if (sv) sv[i] = x[q];
                const float y = x[q] / d;
                st[i] = y;
                hx[i] = y;
            }
        }
    }
}


template <int R, int RPT, int NW>
__global__ __launch_bounds__(NW == 1 ? kBlock : 64 * NW) void k_orth_wy(OrthArgs a, int nunits) {
    constexpr int kRed = (2 * R + 2) > (2 * R * R) ? (2 * R + 2) : (2 * R * R);  // largest sum
    __shared__ __attribute__((aligned(16))) float red[2 * (NW + 1) * kRed];
    constexpr int NT = 64 * NW;  // threads per panel
    const int unit = NW == 1 ? blockIdx.x * kWaves + (threadIdx.x >> 6) : blockIdx.x;
    if (unit >= nunits) return;  // NW == 1 only: whole waves leave, no barrier follows
    const OrthUnit u = a.units[unit];
    if (u.r == 1) {
        joint_norm_grp<NW>(a, u, red);
        return;
    }
    PSGD_STAMP(0);
    const int r = u.r;
    const int k = int(u.k);
    const int t = NW == 1 ? (threadIdx.x & 63) : threadIdx.x;
    const int nq = (k + NT - 1) / NT;  // row slots in use (uniform); slot q holds row t + q*NT
    float* __restrict__ st = a.state + u.off;
    float* __restrict__ sv = a.save ? a.save + u.off : nullptr;
    // Rows >= k are zero, so they add nothing to any sum and stay zero under every update;
    // rows in slots q >= 1 are >= NT > R, i.e. strictly below every diagonal element: only
    // slot 0 needs the diagonal cases (i == j / i < j).
    float A[RPT][R];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {  // whole rows, from clamped (always valid) row indices
        const int i = t + q * NT;
        ld_row<R>(st + int64_t(i < k ? i : 0) * r, r, A[q]);
    }
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int i = t + q * NT;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            keep(A[q][c]);
            A[q][c] = i < k ? A[q][c] : 0.f;
        }
    }
    if (sv) {
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int i = t + q * NT;
            if (q < nq && i < k) st_row<R>(sv + int64_t(i) * r, r, A[q]);
        }
    }
    PSGD_STAMP(1);
    int phase = 0;
    float tau[R];
    // ---- geqr2: A <- R (rows < r) and V (strictly below the diagonal, unit diagonal implied)
#pragma unroll
    for (int j = 0; j < R; ++j) {
        tau[j] = 0.f;
        if (j >= r) continue;
        // v[0] = sum_{i>j} A[i][j]^2, v[1] = alpha, v[2+c] = d_c (c > j), v[2+R+c] = A[j][c] (c > j)
        float v[2 + 2 * R];
#pragma unroll
        for (int e = 0; e < 2 + 2 * R; ++e) v[e] = 0.f;
        {
            const float x = A[0][j];
            const float xb = t > j ? x : 0.f;
            v[0] = xb * xb;
            v[1] = t == j ? x : 0.f;
#pragma unroll
            for (int c = j + 1; c < R; ++c) {
                v[2 + c] = xb * A[0][c];
                v[2 + R + c] = t == j ? A[0][c] : 0.f;
            }
        }
#pragma unroll
        for (int q = 1; q < RPT; ++q) {
            if (q < nq) {  // uniform: unused row slots do nothing
                const float x = A[q][j];
                v[0] = fmaf(x, x, v[0]);
    #pragma unroll
                for (int c = j + 1; c < R; ++c) v[2 + c] = fmaf(x, A[q][c], v[2 + c]);
            }
        }
        grp_sum<2 + 2 * R, NW, kRed>(v, red, phase);
        const float alpha = v[1];
        if (v[0] != 0.f) {  // LAPACK slarfg: xnorm == 0 -> tau = 0, H_j = I
            const float beta = -copysignf(hypotf(alpha, sqrtf(v[0])), alpha);
            const float tj = (beta - alpha) / beta;
            const float scal = 1.f / (alpha - beta);
            tau[j] = tj;
            float w[R];
#pragma unroll
            for (int c = j + 1; c < R; ++c) w[c] = v[2 + R + c] + scal * v[2 + c];
            {
                const bool below = t > j;
                const float vi = below ? A[0][j] * scal : (t == j ? 1.f : 0.f);
                A[0][j] = below ? vi : (t == j ? beta : A[0][j]);
#pragma unroll
                for (int c = j + 1; c < R; ++c) A[0][c] -= tj * vi * w[c];
            }
#pragma unroll
            for (int q = 1; q < RPT; ++q) {
                if (q < nq) {  // uniform: unused row slots do nothing
                    const float vi = A[q][j] * scal;
                    A[q][j] = vi;
    #pragma unroll
                    for (int c = j + 1; c < R; ++c) A[q][c] -= tj * vi * w[c];
                }
            }
        }
    }
    PSGD_STAMP(40);
    // ---- slarft: T from tau and S = V^T V; V1 = rows 0..r-1 of V, broadcast in the same sum
    float sv2[2 * R * R];  // [0, R*R): S[a][b] (a < b); [R*R, 2R*R): V[row a][col b]
#pragma unroll
    for (int e = 0; e < 2 * R * R; ++e) sv2[e] = 0.f;
    {
        float vr[R];  // row t of V (slot 0 holds the diagonal cases)
#pragma unroll
        for (int c = 0; c < R; ++c) vr[c] = (c < r) ? (t == c ? 1.f : (t > c ? A[0][c] : 0.f)) : 0.f;
#pragma unroll
        for (int a2 = 0; a2 < R; ++a2)
#pragma unroll
            for (int b = a2 + 1; b < R; ++b) sv2[a2 * R + b] = vr[a2] * vr[b];
#pragma unroll
        for (int a2 = 0; a2 < R; ++a2)
#pragma unroll
            for (int b = 0; b < R; ++b) sv2[R * R + a2 * R + b] = t == a2 ? vr[b] : 0.f;
    }
#pragma unroll
    for (int q = 1; q < RPT; ++q) {
        if (q < nq) {  // uniform: unused row slots do nothing
    #pragma unroll
            for (int a2 = 0; a2 < R; ++a2)
    #pragma unroll
                for (int b = a2 + 1; b < R; ++b) sv2[a2 * R + b] = fmaf(A[q][a2], A[q][b], sv2[a2 * R + b]);
        }
    }
    grp_sum<2 * R * R, NW, kRed>(sv2, red, phase);
    float T[R][R];
#pragma unroll
    for (int a2 = 0; a2 < R; ++a2)
#pragma unroll
        for (int b = 0; b < R; ++b) T[a2][b] = 0.f;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (j >= r) continue;
        // T[0:j, j] = -tau_j * T[0:j, 0:j] * S[0:j, j];  T[j][j] = tau_j
        float y[R];
#pragma unroll
        for (int a2 = 0; a2 < R; ++a2) y[a2] = a2 < j ? -tau[j] * sv2[a2 * R + j] : 0.f;
#pragma unroll
        for (int a2 = 0; a2 < R; ++a2) {
            if (a2 >= j) continue;
            float acc = 0.f;
#pragma unroll
            for (int b = 0; b < R; ++b)
                if (b >= a2 && b < j) acc = fmaf(T[a2][b], y[b], acc);
            T[a2][j] = acc;
        }
        T[j][j] = tau[j];
    }
    // M = T V1^T  (r x r):  M[l][c] = sum_b T[l][b] * V[c][b]
    float M[R][R];
#pragma unroll
    for (int l = 0; l < R; ++l)
#pragma unroll
        for (int c = 0; c < R; ++c) {
            float acc = 0.f;
#pragma unroll
            for (int b = 0; b < R; ++b) acc = fmaf(T[l][b], sv2[R * R + c * R + b], acc);
            M[l][c] = acc;
        }
    // Q[i][c] = [i == c] - sum_l V[i][l] * M[l][c]
    float* __restrict__ hx = a.hx + u.off;
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        if (q < nq) {  // uniform: unused row slots do nothing
            const int i = t + q * NT;
            float vr[R];
    #pragma unroll
            for (int c = 0; c < R; ++c) {
                if (q == 0)
                    vr[c] = (c < r) ? (i == c ? 1.f : (i > c ? A[0][c] : 0.f)) : 0.f;
                else
                    vr[c] = A[q][c];  // c >= r columns are zero
            }
            float qrow[R];
    #pragma unroll
            for (int c = 0; c < R; ++c) {
                float acc = 0.f;
    #pragma unroll
                for (int l = 0; l < R; ++l) acc = fmaf(vr[l], M[l][c], acc);
                qrow[c] = (i == c ? 1.f : 0.f) - acc;
            }
            if (i < k) {
                st_row<R>(st + int64_t(i) * r, r, qrow);
                st_row<R>(hx + int64_t(i) * r, r, qrow);
            }
        }
    }
    PSGD_STAMP(42);
}

// ------------------------------------------------ paper-code Gram-Schmidt (variant) ----
// paper-code/gradient_reducers.py:945-956 (RankKReducer / HalfRankKReducer), per matrix:
//   for i: col_i /= sqrt(sum col_i^2) + 1e-8 ; rest -= (col_i . rest) col_i
// (the eps is ADDED to the norm, unlike the reference codec's max(norm, eps)). One
// workgroup per panel, in place, column sums as fixed-order workgroup reductions.
template <int R>
__global__ __launch_bounds__(kBlock) void k_orth_mgs(OrthArgs a) {
    __shared__ float red[kWaves * R];
    const OrthUnit u = a.units[blockIdx.x];
    const int r = u.r;
    const int64_t k = u.k;
    const int tid = threadIdx.x;
    float* __restrict__ x = a.state + u.off;
    for (int i = 0; i < r; ++i) {
        float s1[1] = {0.f};
        for (int64_t row = tid; row < k; row += kBlock) {
            const float v = x[row * r + i];
            s1[0] = fmaf(v, v, s1[0]);
        }
        block_sum_nw<float, 1, kWaves>(s1, red);
        const float den = sqrtf(s1[0]) + 1e-8f;
        for (int64_t row = tid; row < k; row += kBlock) x[row * r + i] = x[row * r + i] / den;
        __syncthreads();
        if (i + 1 < r) {
            float dt[R];
#pragma unroll
            for (int c = 0; c < R; ++c) dt[c] = 0.f;
            for (int64_t row = tid; row < k; row += kBlock) {
                const float ci = x[row * r + i];
#pragma unroll
                for (int c = 0; c < R; ++c)
                    if (c > i && c < r) dt[c] = fmaf(ci, x[row * r + c], dt[c]);
            }
            block_sum_nw<float, R, kWaves>(dt, red);
            for (int64_t row = tid; row < k; row += kBlock) {
                const float ci = x[row * r + i];
#pragma unroll
                for (int c = 0; c < R; ++c)
                    if (c > i && c < r) x[row * r + c] -= dt[c] * ci;
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------ selection and instance tables ----
enum class OrthKernel { Wy, Reg, Lds };
struct OrthChoice {
    OrthKernel kernel;
    int rpt, nw;         // Wy / Reg: rows per thread, waves per panel
    int64_t lds_floats;  // Lds: dynamic LDS floats
};

// register budget of the WY kernel (checked with -Rpass-analysis=kernel-resource-usage:
// no spills for these pairs at the launch bounds used)
__host__ __device__ constexpr bool orth_wy_ok(int R, int RPT) {
    return R <= 4 ? R * RPT <= 32 : R * RPT <= 16;
}

// Register budget: 1024-thread workgroups get at most 128 VGPRs, so the panel slice a
// thread holds is capped as below (no spills for any instantiated pair).
// (checked with -Rpass-analysis=kernel-resource-usage: ranks 16/32 spill, so they take the
// LDS kernel above).
__host__ __device__ constexpr bool orth_reg_ok(int R, int RPT) {
    return R == 1 || (R <= 4 && R * RPT <= 32) || (R == 8 && RPT <= 2);
}

// The Householder kernel of a plan whose rank bucket is R (a power of two, > 1) and whose
// longest panel has kmax rows. Everything below is derived from this one function.
__host__ __device__ constexpr OrthChoice orth_select(int R, int64_t kmax) {
    // the fast WY kernel when the panel slice fits in registers. Waves per panel: as few as
    // keep every wave at <= 8 rows (1 wave up to 512 rows ... 16 waves up to 8192 rows).
    if (R == 2 || R == 4 || R == 8) {
        // R = 8 needs > 128 VGPRs: no 1024-thread groups (R = 8 x 1024 threads spills)
        const int nw_max = R == 8 ? 8 : 16;
        int nw = 1;
        while (nw < nw_max && int64_t(64) * nw * 8 < kmax) nw = nw == 1 ? 4 : nw * 2;
        int64_t rpt = 1;
        while (rpt * 64 * nw < kmax) rpt <<= 1;
        if (rpt <= 8 && orth_wy_ok(R, int(rpt))) return {OrthKernel::Wy, int(rpt), nw, 0};
        // register-resident path when the longest panel fits RPT * R <= 128 floats/thread
        rpt = 1;
        while (rpt * kOrthThreads < kmax) rpt <<= 1;
        if (rpt <= 16 && orth_reg_ok(R, int(rpt))) return {OrthKernel::Reg, int(rpt), kOrthWaves, 0};
    }
    constexpr int64_t kLdsCap = 60 * 1024 / 4;  // dynamic LDS floats (stays under the 64 KiB default)
    const int64_t panel = kmax * R;
    return {OrthKernel::Lds, 0, 0, panel < kLdsCap ? panel : kLdsCap};
}

// An instance is built iff the selection picks it for the longest panel it can hold, 64 NW RPT
// rows (k_orth_reg: NW = 16). k_orth_reg<1, 1> is the rank-1 joint norm of every plan.
__host__ __device__ constexpr bool orth_built(OrthKernel kn, int R, int RPT, int NW) {
    if (R == 1) return kn == OrthKernel::Reg && RPT == 1;
    const OrthChoice c = orth_select(R, int64_t(64) * NW * RPT);
    return c.kernel == kn && c.rpt == RPT && c.nw == NW;
}
// Every panel length selects a built instance: the thresholds of orth_select are powers of
// two, so each power of two and its successor cover every case.
__host__ __device__ constexpr bool orth_selection_built() {
    for (int R = 2; R <= 8; R *= 2)
        for (int64_t p = 1; p <= (int64_t(1) << 20); p <<= 1)
            for (int64_t kmax = p; kmax <= p + 1; ++kmax) {
                const OrthChoice c = orth_select(R, kmax);
                if (c.kernel != OrthKernel::Lds && !orth_built(c.kernel, R, c.rpt, c.nw)) return false;
            }
    return true;
}
static_assert(orth_selection_built(), "orth_select picks a kernel instance that is not built");

// A launcher reached with a pair that has no instance fails: it never skips the launch.
template <int R, int RPT, int NW>
hipError_t launch_orth_wy_one(const OrthArgs& a, int nunits, hipStream_t s) {
    if constexpr (orth_built(OrthKernel::Wy, R, RPT, NW)) {
        const int blocks = NW == 1 ? (nunits + kWaves - 1) / kWaves : nunits;
        k_orth_wy<R, RPT, NW><<<blocks, NW == 1 ? kBlock : 64 * NW, 0, s>>>(a, nunits);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

template <int R, int NW>
hipError_t launch_orth_wy_r(int rpt, const OrthArgs& a, int nunits, hipStream_t s) {
    switch (rpt) {
        case 1: return launch_orth_wy_one<R, 1, NW>(a, nunits, s);
        case 2: return launch_orth_wy_one<R, 2, NW>(a, nunits, s);
        case 4: return launch_orth_wy_one<R, 4, NW>(a, nunits, s);
        case 8: return launch_orth_wy_one<R, 8, NW>(a, nunits, s);
        default: return hipErrorInvalidValue;
    }
}

template <int R>
hipError_t launch_orth_wy(int rpt, int nw, const OrthArgs& a, int nunits, hipStream_t s) {
    switch (nw) {
        case 1: return launch_orth_wy_r<R, 1>(rpt, a, nunits, s);
        case 4: return launch_orth_wy_r<R, 4>(rpt, a, nunits, s);
        case 8: return launch_orth_wy_r<R, 8>(rpt, a, nunits, s);
        case 16: return launch_orth_wy_r<R, 16>(rpt, a, nunits, s);
        default: return hipErrorInvalidValue;
    }
}

template <int R, int RPT>
hipError_t launch_orth_reg_one(const OrthArgs& a, int nunits, hipStream_t s) {
    if constexpr (orth_built(OrthKernel::Reg, R, RPT, kOrthWaves)) {
        k_orth_reg<R, RPT><<<nunits, kOrthThreads, 0, s>>>(a);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

template <int R>
hipError_t launch_orth_reg(int rpt, const OrthArgs& a, int nunits, hipStream_t s) {
    switch (rpt) {
        case 1: return launch_orth_reg_one<R, 1>(a, nunits, s);
        case 2: return launch_orth_reg_one<R, 2>(a, nunits, s);
        case 4: return launch_orth_reg_one<R, 4>(a, nunits, s);
        case 8: return launch_orth_reg_one<R, 8>(a, nunits, s);
        case 16: return launch_orth_reg_one<R, 16>(a, nunits, s);
        default: return hipErrorInvalidValue;
    }
}

// the LDS / in-place kernel: ranks 16 and 32 always, ranks 2 to 8 past the register kernels
inline hipError_t launch_orth_lds(int R, const OrthArgs& a, int nunits, int64_t lds_floats, hipStream_t s) {
    const size_t bytes = size_t(lds_floats) * sizeof(float);
    switch (R) {
        case 2: k_orth<2><<<nunits, kBlock, bytes, s>>>(a, lds_floats); break;
        case 4: k_orth<4><<<nunits, kBlock, bytes, s>>>(a, lds_floats); break;
        case 8: k_orth<8><<<nunits, kBlock, bytes, s>>>(a, lds_floats); break;
        case 16: k_orth<16><<<nunits, kBlock, bytes, s>>>(a, lds_floats); break;
        case 32: k_orth<32><<<nunits, kBlock, bytes, s>>>(a, lds_floats); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace psgd
