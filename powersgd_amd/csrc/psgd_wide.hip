// Effective ranks 33-128 (rank bucket 64 / 128) for fp32 and bf16 gradients. The kernels of
// psgd_stream.cuh / psgd_even.cuh hold a row's r accumulators per lane, which stops at 32; here
// every product runs on the exact fp32 matrix instruction v_mfma_f32_16x16x4_f32, and nothing is
// fused (psgd_step.cpp: compress_wide / decompress_wide):
//
//   k_wide_product<EVEN>  Q_part = G_k^T X per (64-column block, row chunk) tile
//   k_wide_product<ODD>   P_part = G_k X   per (64-row block, column strip) tile
//                                                            reference powersgd.py:185-193
//   k_wide_reduce         fixed-order sum of the partials -> state + history copy (no atomics)
//   k_wide_apply          residual = G_0 - sum_k P_k Q_k^T, output = alpha sum_k P_k Qbar_k^T
//                                                            reference powersgd.py:195-230
//   k_wide_gram / k_wide_chol / k_wide_orth_apply
//                         Cholesky-QR with LAPACK's column signs in three launches (below);
//                         rank-1 groups the joint norm     reference orthogonalization.py:4-8
//
// The error-feedback matrix is formed per element on the matrix core (the per-element form):
// a wave holds a 16 x 16 sub-tile of G_0 in the accumulator layout and subtracts P_j Q_j^T with
// r / 4 MFMAs per term, exactly the reference's baddbmm_ (:195-202) up to the order of the r
// products of one element. That tile is then the A operand of the product with the in-factor.
//
// Layouts (cdna_hip_programming.md, v_mfma_f32_16x16x4_f32; lane l = (ri = l & 15, kq = l >> 4)):
// A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k, D[i][j] in lane j + 16 (i / 4), item i % 4.
// With `o` the out-factor index (even: matrix column, odd: matrix row) and `s` the summed one,
// a lane's four accumulator items are Gk(o0 + ri, s0 + 4 kq + i): D[4 kq + i][ri] of
// (-FS)[16 x 4] . FO^T[4 x 16] (FS / FO: the term's factor on the s / o side). The same four
// values are the A operands (row ri, k = kq) of four products whose B operand is
// X[s0 + 4 kq + i][c]; output column c = 64 T + 4 ri + t of MFMA t, so the in-factor row is one
// 16-byte load per four MFMAs and a lane ends with four contiguous columns of four out rows.
// The k index of every MFMA is a permutation of the summed index, identical on both operands.
// Columns c >= r of a narrower matrix in the bucket, rows past the matrix and past the tile are
// zero operands.
#include <hip/hip_runtime.h>

#include "psgd.h"
#include "psgd_chain.cuh"

namespace psgd {

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float g2f(float v) { return v; }
__device__ __forceinline__ float g2f(bf16_t v) { return bf2f(v); }
__device__ __forceinline__ void f2g(float* p, float v) { *p = v; }
__device__ __forceinline__ void f2g(bf16_t* p, float v) { *p = f2bf(v); }  // round to nearest even

// four consecutive gradient elements of one row (16 / 8 aligned bytes)
__device__ __forceinline__ f32x4_t ld_g4(const float* p) { return *reinterpret_cast<const f32x4_t*>(p); }
__device__ __forceinline__ f32x4_t ld_g4(const bf16_t* p) {
    const v2u x = *reinterpret_cast<const v2u*>(p);
    return f32x4_t{__uint_as_float(x[0] << 16), __uint_as_float(x[0] & 0xffff0000u), __uint_as_float(x[1] << 16),
                   __uint_as_float(x[1] & 0xffff0000u)};
}
__device__ __forceinline__ void st_g4(float* p, const f32x4_t& v) { *reinterpret_cast<f32x4_t*>(p) = v; }
__device__ __forceinline__ void st_g4(bf16_t* p, const f32x4_t& v) {
    const v2u x = {uint32_t(f2bf(v[0])) | (uint32_t(f2bf(v[1])) << 16), uint32_t(f2bf(v[2])) | (uint32_t(f2bf(v[3])) << 16)};
    *reinterpret_cast<v2u*>(p) = x;
}

// factor values F[row][c .. c + 3] of an [*, r] panel (zero past r or when !rowok); vec: r % 4 ==
// 0 and the panel is 16-byte aligned (c is always a multiple of 4)
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

// Gradient sub-tile in the accumulator layout: items i = G(o, s4 + i), zero outside the matrix
// and past `send`. ROWS_O: o is the matrix row (odd product, apply: four consecutive elements of
// one row); else o is the column (even product: four rows, one element each; across the 16
// lanes of a row group and the four waves of the workgroup a row's 256 bytes are contiguous).
template <typename T, bool ROWS_O>
__device__ __forceinline__ f32x4_t ld_gtile(const T* __restrict__ G, int64_t n, int64_t m, int64_t o, int64_t s4,
                                            int64_t send, bool vec) {
    f32x4_t g = {0.f, 0.f, 0.f, 0.f};
    if constexpr (ROWS_O) {
        if (o < n && s4 < send) {
            const T* p = G + o * m + s4;
            if (vec && s4 + 3 < send) {
                g = ld_g4(p);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (s4 + i < send) g[i] = g2f(p[i]);
            }
        }
    } else {
        if (o < m) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (s4 + i < send) g[i] = g2f(G[(s4 + i) * m + o]);
        }
    }
    return g;
}

// g[u] += sign * (FS FO^T) for the four 16 x 16 sub-tiles u of a lane's step: FO rows o (one per
// ri), FS rows s0 + 16 u + ri
template <int R, bool NEG>
__device__ __forceinline__ void term_tiles(f32x4_t (&g)[4], const float* __restrict__ FO, const float* __restrict__ FS,
                                           int64_t o, bool ook, int64_t s0, int64_t send, int ri, int kq, int r) {
    const bool vo = fac_vec(FO, r), vs = fac_vec(FS, r);
#pragma unroll
    for (int cc = 0; cc < R; cc += 16) {
        if (cc < r) {  // wave-uniform
            const f32x4_t fo = ld_fac4(FO, o, ook, cc + 4 * kq, r, vo);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t srow = s0 + 16 * u + ri;
                const f32x4_t fs = ld_fac4(FS, srow, srow < send, cc + 4 * kq, r, vs);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    g[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(NEG ? -fs[e] : fs[e], fo[e], g[u], 0, 0, 0);
            }
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------ products --
template <typename T, int R, bool EVEN>
__global__ __launch_bounds__(kBlock) void k_wide_product(WideArgs a) {
    constexpr int NT = R / 64;  // 64-column groups of the in-factor
    const Tile t = a.tiles[blockIdx.x];
    const MatDesc d = a.mats[t.mat];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ri = lane & 15, kq = lane >> 4;
    const int r = d.r;
    const int64_t n = d.n, m = d.m;
    const int64_t O = EVEN ? m : n, S = EVEN ? n : m;
    const int64_t o0 = int64_t(EVEN ? t.strip : t.chunk) * kWideOut + 16 * wave;
    if (o0 >= O) return;  // wave-uniform (the kernel has no workgroup barrier)
    const int64_t schunk = EVEN ? d.chunk_rows : d.odd_sw;  // a multiple of kWideStep
    const int ci = EVEN ? t.chunk : t.strip;
    const int64_t sbeg = ci * schunk;
    const int64_t send = S < sbeg + schunk ? S : sbeg + schunk;
    const T* __restrict__ G = static_cast<const T*>(a.grads[t.tensor]);
    const bool gvec = !EVEN && m % 4 == 0 && reinterpret_cast<uintptr_t>(G) % (4 * sizeof(T)) == 0;
    const float* __restrict__ X = a.x + (EVEN ? d.poff : d.qoff);
    const bool vx = fac_vec(X, r);
    const int64_t o = o0 + ri;
    const bool ook = o < O;

    f32x4_t acc[NT * 4];
#pragma unroll
    for (int q = 0; q < NT * 4; ++q) acc[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int64_t s0 = sbeg; s0 < send; s0 += kWideStep) {
        f32x4_t g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) g[u] = ld_gtile<T, !EVEN>(G, n, m, o, s0 + 16 * u + 4 * kq, send, gvec);
        for (int k = 0; k < a.nres; ++k) {  // G_k = G_0 - sum_j P_j Q_j^T (reference :195-202)
            const float* FO = EVEN ? a.res.q[k] + d.qoff : a.res.p[k] + d.poff;
            const float* FS = EVEN ? a.res.p[k] + d.poff : a.res.q[k] + d.qoff;
            term_tiles<R, true>(g, FO, FS, o, ook, s0, send, ri, kq, r);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t srow = s0 + 16 * u + 4 * kq + i;
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) {
                    if (64 * tt < r) {  // wave-uniform
                        const f32x4_t xv = ld_fac4(X, srow, srow < send, 64 * tt + 4 * ri, r, vx);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[tt * 4 + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][i], xv[e], acc[tt * 4 + e], 0, 0, 0);
                    }
                }
            }
    }
    // lane (ri, kq), item j of acc[4 tt + e]: Y[o0 + 4 kq + j][64 tt + 4 ri + e]
    float* __restrict__ dst = a.part + (EVEN ? d.part_even : d.part_odd) + int64_t(ci) * O * r;
    const bool vd = fac_vec(dst, r);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t orow = o0 + 4 * kq + j;
        if (orow >= O) continue;
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            const int c = 64 * tt + 4 * ri;
            if (c >= r) continue;
            float* p = dst + orow * r + c;
            if (vd) {
                *reinterpret_cast<f32x4_t*>(p) =
                    f32x4_t{acc[tt * 4][j], acc[tt * 4 + 1][j], acc[tt * 4 + 2][j], acc[tt * 4 + 3][j]};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < r) p[e] = acc[tt * 4 + e][j];
            }
        }
    }
}

// one workgroup per item of up to kRedItem consecutive factor elements; partials in chunk order
__global__ __launch_bounds__(kBlock) void k_wide_reduce(WideArgs a) {
    const RedItem it = a.items[blockIdx.x];
    if (int(threadIdx.x) >= it.cnt) return;
    const MatDesc d = a.mats[it.mat];
    const int64_t len = (a.even ? d.m : d.n) * d.r;
    const int64_t e = int64_t(it.start) + threadIdx.x;
    const float* __restrict__ p = a.part + (a.even ? d.part_even : d.part_odd) + e;
    float s = p[0];
    for (int c = 1; c < it.np; ++c) s += p[int64_t(c) * len];
    const int64_t off = (a.even ? d.qoff : d.poff) + e;
    a.y[off] = s;
    a.yh[off] = s;
    if (a.xout) st_slot(a.xout + off, s);  // the IPC exchange's hand-off (write-through), as k_reduce
}

// --------------------------------------------------------------------------- apply --
// Tile: 64 rows (16 per wave) x kWideApplyCols columns. SHARED (world size 1): the local and the
// all-reduced factors are the same buffers and alpha = 1: one accumulation S = sum_k P_k Q_k^T
// gives output = S and residual = G_0 - S. Otherwise the residual accumulator starts from G_0
// and the local terms are subtracted on the matrix core, the output accumulates the
// all-reduced terms from zero.
template <typename T, int R, bool SHARED>
__global__ __launch_bounds__(kBlock) void k_wide_apply(WideArgs a) {
    const Tile t = a.tiles[blockIdx.x];
    const MatDesc d = a.mats[t.mat];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ri = lane & 15, kq = lane >> 4;
    const int r = d.r;
    const int64_t n = d.n, m = d.m;
    const int64_t o0 = int64_t(t.chunk) * kWideOut + 16 * wave;
    if (o0 >= n) return;  // wave-uniform
    const int64_t sbeg = int64_t(t.strip) * kWideApplyCols;
    const int64_t send = m < sbeg + kWideApplyCols ? m : sbeg + kWideApplyCols;
    T* __restrict__ G = static_cast<T*>(a.grads[t.tensor]);
    T* __restrict__ Out = static_cast<T*>(a.out) + d.out_off;
    const bool gvec = m % 4 == 0 && reinterpret_cast<uintptr_t>(G) % (4 * sizeof(T)) == 0 &&
                      reinterpret_cast<uintptr_t>(Out) % (4 * sizeof(T)) == 0;
    const int64_t o = o0 + ri;
    const bool ook = o < n;
    const float alpha = a.alpha;
    for (int64_t s0 = sbeg; s0 < send; s0 += kWideStep) {
        f32x4_t g[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            g[u] = ld_gtile<T, true>(G, n, m, o, s0 + 16 * u + 4 * kq, send, gvec);
            w[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        for (int k = 0; k < a.nres; ++k) {
            if constexpr (SHARED) {
                term_tiles<R, false>(w, a.res.p[k] + d.poff, a.res.q[k] + d.qoff, o, ook, s0, send, ri, kq, r);
            } else {
                term_tiles<R, true>(g, a.res.p[k] + d.poff, a.res.q[k] + d.qoff, o, ook, s0, send, ri, kq, r);   // :195-202
                term_tiles<R, false>(w, a.apx.p[k] + d.poff, a.apx.q[k] + d.qoff, o, ook, s0, send, ri, kq, r);  // :211-219
            }
        }
        if (!ook) continue;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t s4 = s0 + 16 * u + 4 * kq;
            if (s4 >= send) continue;
            f32x4_t res, outv;
            if constexpr (SHARED) {
                res = g[u] - w[u];
                outv = w[u];
            } else {
                res = g[u];
                outv = w[u] * alpha;
            }
            T* gp = G + o * m + s4;
            T* op = Out + o * m + s4;
            if (gvec && s4 + 3 < send) {
                st_g4(gp, res);
                st_g4(op, outv);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (s4 + i < send) {
                        f2g(gp + i, res[i]);
                        f2g(op + i, outv[i]);
                    }
            }
        }
    }
}

// ---------------------------------------------------------------- orthonormalise --
// Q of the Householder QR of each [k, r] panel X with LAPACK's column signs (reference
// orthogonalization.py:8, torch.linalg.qr), computed as Q = X R^-1 D like k_orth_chol /
// orth_chol_wide (psgd_orth_chol.cuh), whose single workgroup per panel cannot hold a 64 / 128
// column chain. Three launches:
//   k_wide_gram        G = X^T X in fp64 on v_mfma_f64_16x16x4_f64, one workgroup per block of
//                      kWideGramRows panel rows (blocks on and above the diagonal, spread over the
//                      four waves); also the `save` copy of the raw panel
//   k_wide_chol        one workgroup per unit: fixed-order sum of the Gram partials, Cholesky
//                      G = R^T R, M = R^-1, T = X[0:r] M and the LU recursion on T that gives
//                      LAPACK's signs D (Ballard et al., as orth_chol_wide), all fp64, the r x r
//                      matrices in LDS (R and M packed upper triangular side by side, then T over
//                      both). Rank-1 units: the joint group norm with max(norm, 1e-16) (:5-6).
//                      A panel the Cholesky rejects (pivot not above 1e-8 of its column's squared
//                      norm: rank-deficient or zero; or a sign pivot within kSignTol of 1) takes
//                      the exact Householder QR here, so a zero panel yields the leading identity
//                      columns.
//   k_wide_orth_apply  Y = X (M D) on the fp64 matrix core over the same row blocks, M D staged in
//                      LDS; writes the state and the history copy.
// f64 MFMA layouts (cdna_hip_programming.md): A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k,
// D[i][j] in lane j + 16 (i % 4), item i / 4.
typedef double f64x4_t __attribute__((ext_vector_type(4)));
constexpr int kWideOrthNT = 1024;

__device__ __forceinline__ float wide_block_sum(float v, float* red) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = red[0];
    for (int w = 1; w < kWideOrthNT / 64; ++w) t += red[w];
    return t;
}

// A[i, c] -= tau v_i w_c for c > j, i >= j, with v = (1, A[j+1:, j]) and w_c = sum_i v_i A[i, c]
template <int R>
__device__ __forceinline__ void wide_reflect(float* A, int64_t k, int r, int j, float tj, float* part, float* wsh) {
    constexpr int NS = kWideOrthNT / R;
    const int c = threadIdx.x % R, s = threadIdx.x / R;
    const bool mine = c > j && c < r;
    float w = 0.f;
    if (mine)
        for (int64_t i = j + 1 + s; i < k; i += NS) w = fmaf(A[i * r + j], A[i * r + c], w);
    part[s * R + c] = w;
    __syncthreads();
    if (s == 0 && mine) {
        float t = part[c];
        for (int q = 1; q < NS; ++q) t += part[q * R + c];
        wsh[c] = t + A[int64_t(j) * r + c];
    }
    __syncthreads();
    if (mine) {
        const float wc = tj * wsh[c];
        for (int64_t i = j + s; i < k; i += NS) {
            const float vi = i == j ? 1.f : A[i * r + j];
            A[i * r + c] -= vi * wc;
        }
    }
    __syncthreads();
}

// Householder QR with LAPACK's geqr2 + org2r conventions (beta = -sign(alpha) ||col||, tau = 0 for
// a column with nothing below the diagonal): the recursion of householder_q (psgd_chain.cuh),
// whose per-thread array of R column sums does not fit the registers at 64 / 128 columns. Thread
// t = (column c = t % R, row slice s = t / R) owns one column sum of one row slice; the slices
// are summed through LDS in slice order. In place in the history buffer A, then copied to st.
template <int R>
__device__ void wide_householder(float* st, float* A, int64_t k, int r, float* part, float* wsh, float* tau, float* red) {
    const int tid = threadIdx.x;
    const int64_t total = k * r;
    for (int64_t i = tid; i < total; i += kWideOrthNT) A[i] = st[i];
    __syncthreads();
    for (int j = 0; j < r; ++j) {  // geqr2
        float s1 = 0.f;
        for (int64_t i = j + 1 + tid; i < k; i += kWideOrthNT) {
            const float x = A[i * r + j];
            s1 = fmaf(x, x, s1);
        }
        s1 = wide_block_sum(s1, red);
        const float alpha = A[int64_t(j) * r + j];
        float tj = 0.f;
        if (s1 != 0.f) {  // workgroup-uniform
            const float beta = -copysignf(hypotf(alpha, sqrtf(s1)), alpha);
            tj = (beta - alpha) / beta;
            const float scal = 1.f / (alpha - beta);
            __syncthreads();  // every thread has read alpha
            for (int64_t i = j + 1 + tid; i < k; i += kWideOrthNT) A[i * r + j] *= scal;
            if (tid == 0) A[int64_t(j) * r + j] = beta;
        }
        if (tid == 0) tau[j] = tj;
        __syncthreads();
        if (tj != 0.f && j + 1 < r) wide_reflect<R>(A, k, r, j, tj, part, wsh);
    }
    for (int j = r - 1; j >= 0; --j) {  // org2r: Q = H_0 .. H_{r-1} I[:, :r], last reflector first
        const float tj = tau[j];
        if (j + 1 < r && tj != 0.f) wide_reflect<R>(A, k, r, j, tj, part, wsh);
        for (int64_t i = j + 1 + tid; i < k; i += kWideOrthNT) A[i * r + j] *= -tj;
        for (int64_t i = tid; i < j; i += kWideOrthNT) A[i * r + j] = 0.f;
        if (tid == 0) A[int64_t(j) * r + j] = 1.f - tj;
        __syncthreads();
    }
    for (int64_t i = tid; i < total; i += kWideOrthNT) st[i] = A[i];
}

template <int R>
__global__ __launch_bounds__(kBlock) void k_wide_gram(WideOrthArgs a) {
    constexpr int NB = R / 16, NBLK = NB * (NB + 1) / 2, PERW = (NBLK + kWaves - 1) / kWaves;
    const Tile t = a.items[blockIdx.x];
    const OrthUnit u = a.units[t.mat];
    const int r = u.r;
    const int64_t k = u.k;
    const float* st = a.state + u.off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ri = lane & 15, kq = lane >> 4;
    const int64_t row0 = int64_t(t.strip) * kWideGramRows;
    const int64_t row1 = k < row0 + kWideGramRows ? k : row0 + kWideGramRows;
    if (a.save)
        for (int64_t e = row0 * r + tid; e < row1 * r; e += kBlock) a.save[u.off + e] = st[e];
    f64x4_t g[PERW];
#pragma unroll
    for (int q = 0; q < PERW; ++q) g[q] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    for (int64_t q0 = row0; q0 < row1; q0 += 4) {
        // lane (ri, kq) = X[q0 + kq][16 cb + ri]: the A operand (A[i][kk] = X[kk][i]) and the B
        // operand (B[kk][j] = X[kk][j]) of a Gram block at once
        const int64_t row = q0 + kq;
        float v[NB];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
            const int c = 16 * cb + ri;
            v[cb] = (row < row1 && c < r) ? st[row * r + c] : 0.f;
        }
        int bl = 0;
#pragma unroll
        for (int ca = 0; ca < NB; ++ca)
#pragma unroll
            for (int cb = ca; cb < NB; ++cb) {
                if ((bl % kWaves) == wave && 16 * cb < r)  // wave-uniform
                    g[bl / kWaves] = __builtin_amdgcn_mfma_f64_16x16x4f64(double(v[ca]), double(v[cb]), g[bl / kWaves], 0, 0, 0);
                ++bl;
            }
    }
    double* dst = a.gram + int64_t(t.chunk) * R * R;
    int bl = 0;
#pragma unroll
    for (int ca = 0; ca < NB; ++ca)
#pragma unroll
        for (int cb = ca; cb < NB; ++cb) {
            if ((bl % kWaves) == wave) {
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[(16 * ca + kq + 4 * e) * R + 16 * cb + ri] = g[bl / kWaves][e];
            }
            ++bl;
        }
}

// packed upper triangle of an R x R matrix: entry (i, j), i <= j
template <int R>
__device__ __forceinline__ int tri(int i, int j) {
    return i * R - (i * (i - 1)) / 2 + (j - i);
}

template <int R>
__global__ __launch_bounds__(kWideOrthNT) void k_wide_chol(WideOrthArgs a) {
    constexpr int NT = kWideOrthNT, TRI = R * (R + 1) / 2, GS = NT / R;
    __shared__ double buf[2 * TRI];  // R | M packed; later T (r x r, stride R)
    __shared__ double gdiag[R];
    __shared__ double sgn[R];
    __shared__ double redd[NT / 64];
    __shared__ float part[NT];
    __shared__ float wsh[R];
    __shared__ float tau[R];
    __shared__ float red[NT / 64];
    __shared__ int ok_sh;
    const OrthUnit u = a.units[blockIdx.x];
    float* st = a.state + u.off;
    float* A = a.hx + u.off;
    const int64_t k = u.k;
    const int r = u.r;
    const int tid = threadIdx.x;
    if (r == 1) {  // a rank-1 shape group: the joint norm, summed in fp64
        const int64_t total = k * u.count;
        if (a.save)
            for (int64_t i = tid; i < total; i += NT) a.save[u.off + i] = st[i];
        double s = 0.0;
        for (int64_t i = tid; i < total; i += NT) s += double(st[i]) * double(st[i]);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((tid & 63) == 0) redd[tid >> 6] = s;
        __syncthreads();
        s = redd[0];
        for (int w = 1; w < NT / 64; ++w) s += redd[w];
        const float nrm = float(sqrt(s));
        const float d = nrm > 1e-16f ? nrm : 1e-16f;  // torch.maximum(norm, eps)
        for (int64_t i = tid; i < total; i += NT) {
            const float x = st[i] / d;
            st[i] = x;
            A[i] = x;
        }
        if (tid == 0) a.ok[blockIdx.x] = 0;
        return;
    }
    double* W = buf;
    double* M = buf + TRI;
    double* T = buf;
    const int nrb = int((k + kWideGramRows - 1) / kWideGramRows);
    const double* gp = a.gram + int64_t(a.slot0[blockIdx.x]) * R * R;
    for (int e = tid; e < r * r; e += NT) {  // Gram partials in row-block order
        const int i = e / r, j = e - i * r;
        if (i <= j) {
            double s = 0.0;
            for (int b = 0; b < nrb; ++b) s += gp[int64_t(b) * R * R + i * R + j];
            W[tri<R>(i, j)] = s;
            if (i == j) gdiag[i] = s;
        }
    }
    if (tid == 0) ok_sh = 1;
    __syncthreads();
    for (int j = 0; j < r; ++j) {  // Cholesky G = R^T R, upper R in place
        const double piv = W[tri<R>(j, j)];
        if (tid == 0 && !(piv > 1e-8 * gdiag[j] && piv > 0.0)) ok_sh = 0;
        const double d = sqrt(piv > 0.0 ? piv : 1.0);
        __syncthreads();
        if (tid > j && tid < r) W[tri<R>(j, tid)] /= d;
        if (tid == j) W[tri<R>(j, j)] = d;
        __syncthreads();
        const int nn = r - j - 1;
        for (int e = tid; e < nn * nn; e += NT) {
            const int i = j + 1 + e / nn, b = j + 1 + e % nn;
            if (b >= i) W[tri<R>(i, b)] -= W[tri<R>(j, i)] * W[tri<R>(j, b)];
        }
        __syncthreads();
    }
    if (ok_sh) {  // workgroup-uniform
        // M = R^-1 by back substitution: GS lanes share column c and split the sum over l
        const int c = tid / GS, sub = tid % GS;
        const bool col = c < r;
        for (int i = r - 1; i >= 0; --i) {
            double p = 0.0;
            if (col && c >= i)
                for (int l = i + 1 + sub; l <= c; l += GS) p += W[tri<R>(i, l)] * M[tri<R>(l, c)];
            for (int o = GS / 2; o > 0; o >>= 1) p += __shfl_xor(p, o);
            if (col && c >= i && sub == 0) M[tri<R>(i, c)] = ((i == c ? 1.0 : 0.0) - p) / W[tri<R>(i, i)];
            __syncthreads();
        }
        double* mg = a.m + int64_t(blockIdx.x) * R * R;
        for (int e = tid; e < R * R; e += NT) {
            const int l = e / R, cc = e - l * R;
            mg[e] = (l <= cc && cc < r) ? M[tri<R>(l, cc)] : 0.0;
        }
        __syncthreads();  // M is in global memory from here on; T takes the LDS
        for (int e = tid; e < r * r; e += NT) {  // T = X[0:r] M
            const int i = e / r, cc = e - i * r;
            double v = 0.0;
            for (int l = 0; l <= cc; ++l) v += double(st[int64_t(i) * r + l]) * mg[l * R + cc];
            T[i * R + cc] = v;
        }
        __syncthreads();
        for (int j = 0; j < r; ++j) {  // LAPACK's column signs: the LU recursion of orth_chol_wide
            const double tjj = T[j * R + j];
            const bool nonneg = tjj >= 0.0;
            if (tid == 0 && j < k - 1 && fabs(tjj) > 1.0 - kSignTol) ok_sh = 0;
            const double sj = (j == k - 1) ? (nonneg ? 1.0 : -1.0) : (nonneg ? -1.0 : 1.0);
            if (tid == 0) sgn[j] = sj;
            const double piv = tjj - sj;
            const int nn = r - j - 1;
            for (int e = tid; e < nn * nn; e += NT) {
                const int i = j + 1 + e / nn, b = j + 1 + e % nn;
                T[i * R + b] -= (T[i * R + j] / piv) * T[j * R + b];
            }
            __syncthreads();
        }
    }
    if (!ok_sh) {  // exact Householder QR (the save copy was made by k_wide_gram)
        wide_householder<R>(st, A, k, r, part, wsh, tau, red);
        if (tid == 0) a.ok[blockIdx.x] = 0;
        return;
    }
    if (tid < R) a.sg[int64_t(blockIdx.x) * R + tid] = tid < r ? sgn[tid] : 0.0;
    if (tid == 0) a.ok[blockIdx.x] = 1;
}

template <int R>
__global__ __launch_bounds__(kBlock) void k_wide_orth_apply(WideOrthArgs a) {
    constexpr int NB = R / 16;
    __shared__ double msh[R * R];  // M' = M D, row-major M'[l][c]
    const Tile t = a.items[blockIdx.x];
    if (!a.ok[t.mat]) return;  // workgroup-uniform: the chain kernel finished this unit itself
    const OrthUnit u = a.units[t.mat];
    const int r = u.r;
    const int64_t k = u.k;
    float* st = a.state + u.off;
    float* hx = a.hx + u.off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ri = lane & 15, kq = lane >> 4;
    const double* mg = a.m + int64_t(t.mat) * R * R;
    const double* sg = a.sg + int64_t(t.mat) * R;
    for (int e = tid; e < R * R; e += kBlock) msh[e] = mg[e] * sg[e % R];
    __syncthreads();
    const int64_t row0 = int64_t(t.strip) * kWideGramRows;
    const int64_t row1 = k < row0 + kWideGramRows ? k : row0 + kWideGramRows;
    // a wave takes 16-row blocks; output block cb, inner block lb <= cb (M' is upper triangular),
    // MFMA e covers inner columns l = 16 lb + 4 kk + e: A[i = ri][kk = kq] = M'[16 lb + 4 kq + e]
    // [16 cb + pi(ri)], pi(i) = 4 (i & 3) + (i >> 2), B[kk = kq][j = ri] = X[b0 + ri][16 lb + 4 kq
    // + e]; the D layout then hands lane (ri, kq), item e, Y[b0 + ri][16 cb + 4 kq + e]
    for (int64_t b0 = row0 + 16 * wave; b0 < row1; b0 += 16 * kWaves) {
        const int64_t row = b0 + ri;
        const bool rok = row < row1;
        float x[NB][4];
#pragma unroll
        for (int lb = 0; lb < NB; ++lb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 16 * lb + 4 * kq + e;
                x[lb][e] = (rok && c < r) ? st[row * r + c] : 0.f;
            }
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
            if (16 * cb >= r) continue;  // wave-uniform
            f64x4_t y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int lb = 0; lb <= cb; ++lb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double am = msh[(16 * lb + 4 * kq + e) * R + 16 * cb + 4 * (ri & 3) + (ri >> 2)];
                    y = __builtin_amdgcn_mfma_f64_16x16x4f64(am, double(x[lb][e]), y, 0, 0, 0);
                }
            if (rok) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = 16 * cb + 4 * kq + e;
                    if (c < r) {
                        st[row * r + c] = float(y[e]);
                        hx[row * r + c] = float(y[e]);
                    }
                }
            }
        }
    }
}

template <int R>
static hipError_t wide_orth_r(const WideOrthArgs& a, int nunits, int nitems, hipStream_t s) {
    if (nitems > 0) k_wide_gram<R><<<nitems, kBlock, 0, s>>>(a);
    k_wide_chol<R><<<nunits, kWideOrthNT, 0, s>>>(a);
    if (nitems > 0) k_wide_orth_apply<R><<<nitems, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_wide_orth(int R, const WideOrthArgs& a, int nunits, int nitems, hipStream_t s) {
    if (nunits == 0) return hipSuccess;
    if (R == 64) return wide_orth_r<64>(a, nunits, nitems, s);
    if (R == 128) return wide_orth_r<128>(a, nunits, nitems, s);
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------- launchers ----
template <typename T>
static hipError_t wide_product_t(int R, bool even, const WideArgs& a, int ntiles, hipStream_t s) {
    if (R == 64) {
        if (even) k_wide_product<T, 64, true><<<ntiles, kBlock, 0, s>>>(a);
        else k_wide_product<T, 64, false><<<ntiles, kBlock, 0, s>>>(a);
    } else if (R == 128) {
        if (even) k_wide_product<T, 128, true><<<ntiles, kBlock, 0, s>>>(a);
        else k_wide_product<T, 128, false><<<ntiles, kBlock, 0, s>>>(a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_wide_product(int dtype, int R, bool even, const WideArgs& a, int ntiles, hipStream_t s) {
    if (ntiles == 0) return hipSuccess;
    return dtype == PSGD_F32 ? wide_product_t<float>(R, even, a, ntiles, s) : wide_product_t<bf16_t>(R, even, a, ntiles, s);
}

hipError_t launch_wide_reduce(const WideArgs& a, int nitems, hipStream_t s) {
    if (nitems == 0) return hipSuccess;
    k_wide_reduce<<<nitems, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

template <typename T>
static hipError_t wide_apply_t(int R, const WideArgs& a, int ntiles, hipStream_t s) {
    const dim3 grid(ntiles), block(kBlock);
    if (R == 64) {
        if (a.shared) timed_launch(k_wide_apply<T, 64, true>, grid, block, s, a);
        else timed_launch(k_wide_apply<T, 64, false>, grid, block, s, a);
    } else if (R == 128) {
        if (a.shared) timed_launch(k_wide_apply<T, 128, true>, grid, block, s, a);
        else timed_launch(k_wide_apply<T, 128, false>, grid, block, s, a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_wide_apply(int dtype, int R, const WideArgs& a, int ntiles, hipStream_t s) {
    if (ntiles == 0) return hipSuccess;
    return dtype == PSGD_F32 ? wide_apply_t<float>(R, a, ntiles, s) : wide_apply_t<bf16_t>(R, a, ntiles, s);
}

}  // namespace psgd
