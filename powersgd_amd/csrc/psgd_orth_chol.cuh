// Cholesky-QR orthonormalisation kernels (k_orth_chol, k_orth_chol16/32, k_orth_chain), their
// build-time defaults and their instance table. Included by psgd_orth.hip only.
#pragma once

#include "psgd_orth_householder.cuh"  // PSGD_STAMP, orth_joint_norm, psgd_chain.cuh

namespace psgd {

// ------------------------------------------- Cholesky QR with LAPACK signs (fast path) ----
// Q of the Householder QR of a k x r panel X (reference orthogonalization.py:8,
// torch.linalg.qr) computed as Q = X R^-1 D:
//   * Gram G = X^T X accumulated in fp64 (one pass over the panel, ONE workgroup
//     reduction) and its Cholesky factor R (fp64, every thread redundantly);
//   * D = the column signs LAPACK's geqr2 gives (beta = -sign(alpha) ||x||, and beta =
//     alpha for a reflector with nothing below the diagonal): read off the top r x r block
//     of X R^-1 by the LU recursion of Ballard et al., "Reconstructing Householder vectors
//     from Tall-Skinny QR" (s_j = -sign(pivot_j); last column of a square panel: +sign);
//   * Q = X (R^-1 D) row by row (fp64, rounded once to fp32).
// With the Gram in fp64, the loss of orthogonality is ~kappa^2 * 1e-16: below fp32
// rounding for kappa < 1e4. A panel with a pivot under 1e-8 of its column's squared norm
// (kappa >~ 1e4, a zero or rank-deficient panel) takes the exact Householder path instead
// (householder_q of psgd_chain.cuh, in place in the history buffer), so zero panels still give the
// leading identity columns. One workgroup per panel, no register-resident panel: the
// second pass re-reads it from L2.
template <int NV, int NW>
__device__ __forceinline__ void block_sum_f64(double (&v)[NV], double* red) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_allsum_f64(v[i]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double t = red[i];
        for (int w = 1; w < NW; ++w) t += red[w * NV + i];
        v[i] = t;
    }
}

// NT threads per panel: 512 for r <= 4 (a 4096-row panel is one batch of loads per pass;
// the kernel is latency-bound, one workgroup per panel), 256 for r = 8 (registers).
template <int R>
struct CholNT {
    static constexpr int value = R <= 4 ? 512 : 256;
};

// RC = R: the panel has exactly R columns (compile-time rank: the r x r arithmetic is
// branch-free straight-line fp64 that the compiler interleaves; it is a serial latency
// chain per workgroup, so this matters); RC = 0: any r <= R at run time.
// rows per thread per load batch of k_orth_chol (ranks 2 / 4). Larger batches (fewer round
// trips on long panels) measured slower: 16 / 12 rows, k_orth_chol<2> 8.5 -> 9.5 us (cfg4),
// <4> 6.3 -> 6.8 us (profiles/r04/t); likewise the whole panel held in registers (r04/l)
#ifndef PSGD_CHOL_U2
#define PSGD_CHOL_U2 8
#endif
// panels of one load batch keep their rows in registers for the second pass (no L2 re-read):
// rank 4 only (k_orth_chol<4> 6.48 -> 6.26 us on cfg3's P panels; rank 2 +0.3 us on cfg4's,
// profiles/r05/orth)
#ifndef PSGD_CHOL_RES
#define PSGD_CHOL_RES 1
#endif
#ifndef PSGD_CHOL_U4
#define PSGD_CHOL_U4 8
#endif

// Gram sums through LDS (NT x NG fp64 partials: 40 KB at rank 4) for r <= 4
template <int R>
constexpr bool kGramLds = R <= 4;

// KU: rows per thread per load batch (0: the PSGD_CHOL_U* default of the rank)
template <int R, int RC, int KU = 0>
__device__ __forceinline__ void orth_chol_panel(const OrthArgs& a, const OrthUnit& u, double* redd, float* red,
                                                float* tau, double* gpart, float* top_sh) {
    constexpr int NG = R * (R + 1) / 2;
    constexpr int NT = CholNT<R>::value;
    const int r = RC > 0 ? RC : u.r;
    const int64_t k = u.k;
    const int tid = threadIdx.x;
    float* __restrict__ st = a.state + u.off;
    float* __restrict__ hx = a.hx + u.off;
    float* __restrict__ sv = a.save ? a.save + u.off : nullptr;

    // rows in batches of kU per thread, all loads of a batch issued together (clamped
    // rows, masked afterwards): the panel was just written by another kernel, so each
    // batch costs one L2/MALL round trip rather than one per row
    constexpr int kU = KU > 0 ? KU : R <= 2 ? PSGD_CHOL_U2 : R <= 4 ? PSGD_CHOL_U4 : 4;
    double g[NG];
#pragma unroll
    for (int e = 0; e < NG; ++e) g[e] = 0.0;
    // PSGD_CHOL_RES: a panel of one batch keeps its rows in registers for the second pass
    constexpr bool kRes = PSGD_CHOL_RES != 0 && (R == 4 || KU > 0);
    const bool res = kRes && k <= int64_t(kU) * NT;
    float xr[kRes ? kU : 1][R];
    for (int64_t i0 = tid; i0 < k; i0 += int64_t(kU) * NT) {
        float x[kU][R];
#pragma unroll
        for (int q = 0; q < kU; ++q) {
            const int64_t i = i0 + int64_t(q) * NT;
            ld_row<R>(st + (i < k ? i : 0) * r, r, x[q]);
        }
#pragma unroll
        for (int q = 0; q < kU; ++q) {
            const int64_t i = i0 + int64_t(q) * NT;
#pragma unroll
            for (int c = 0; c < R; ++c) {
                keep(x[q][c]);
                x[q][c] = i < k ? x[q][c] : 0.f;
            }
            if (sv && i < k) st_row<R>(sv + i * r, r, x[q]);
            if (kGramLds<R> && i < r) {  // the top r rows: the sign recursion's input, from LDS
#pragma unroll
                for (int c = 0; c < R; ++c) top_sh[i * R + c] = x[q][c];
            }
            int e = 0;
#pragma unroll
            for (int c = 0; c < R; ++c)
#pragma unroll
                for (int b = c; b < R; ++b) g[e++] += double(x[q][c]) * double(x[q][b]);
            if constexpr (kRes) {
#pragma unroll
                for (int c = 0; c < R; ++c) xr[q][c] = x[q][c];
            }
        }
    }
    PSGD_STAMP(11);
    if constexpr (kGramLds<R>) {
        // workgroup Gram sums: every thread's NG partials to LDS (entry-major), then wave w
        // sums entries w, w + NW, ... (lane l: threads l, l + 64, ... in order, then the wave
        // tree): at most two fp64 wave reductions per wave instead of NG (the DPP trees of NG
        // fp64 values on every wave were ~40 % of a small panel's kernel time). Fixed order.
        constexpr int NW = NT / 64;
#pragma unroll
        for (int e = 0; e < NG; ++e) gpart[e * NT + tid] = g[e];
        __syncthreads();
        const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int e0 = 0; e0 < NG; e0 += NW) {
            const int e = e0 + wave;
            if (e < NG) {
                double t = gpart[e * NT + lane];
#pragma unroll
                for (int w = 1; w < NW; ++w) t += gpart[e * NT + w * 64 + lane];
                t = wave_allsum_f64(t);
                if (lane == 0) redd[e] = t;
            }
        }
        __syncthreads();
        if ((tid >> 6) == 0) {
#pragma unroll
            for (int e = 0; e < NG; ++e) g[e] = redd[e];
        }
    } else {
        block_sum_f64<NG, NT / 64>(g, redd);
    }
    PSGD_STAMP(12);

    __shared__ double m_sh[R * R];
    __shared__ int ok_sh;
    if ((tid >> 6) == 0) chol_chain<R>(g, kGramLds<R> ? top_sh : nullptr, st, r, k, m_sh, &ok_sh,
                                       a.rfac ? a.rfac + u.off : nullptr);
    __syncthreads();
    PSGD_STAMP(13);
    if (!ok_sh) {  // exact Householder (geqr2 + org2r) in place in the history buffer
        for (int64_t i = tid; i < k * r; i += NT) hx[i] = st[i];
        __syncthreads();
        householder_q<R, NT>(hx, k, r, red, tau, a.rfac ? a.rfac + u.off : nullptr);
        for (int64_t i = tid; i < k * r; i += NT) st[i] = hx[i];
        return;
    }
    double M[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int c = 0; c < R; ++c) M[i][c] = m_sh[i * R + c];
    __syncthreads();  // every thread has read the top block before any row is overwritten
    for (int64_t i0 = tid; i0 < k; i0 += int64_t(kU) * NT) {
        float x[kU][R];
        if (kRes && res) {
#pragma unroll
            for (int q = 0; q < kU; ++q)
#pragma unroll
                for (int c = 0; c < R; ++c) x[q][c] = xr[kRes ? q : 0][c];
        } else {
#pragma unroll
            for (int q = 0; q < kU; ++q) {
                const int64_t i = i0 + int64_t(q) * NT;
                ld_row<R>(st + (i < k ? i : 0) * r, r, x[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < kU; ++q) {
            const int64_t i = i0 + int64_t(q) * NT;
#pragma unroll
            for (int c = 0; c < R; ++c) keep(x[q][c]);
            float y[R];
#pragma unroll
            for (int c = 0; c < R; ++c) {
                double v = 0.0;
#pragma unroll
                for (int l = 0; l < R; ++l) v += double(x[q][l]) * M[l][c];
                y[c] = float(v);
            }
            if (i < k) {
                st_row<R>(st + i * r, r, y);
                st_row<R>(hx + i * r, r, y);
            }
        }
    }
}

// KU > 0: load batches of KU rows per thread (the rank-4 instance for panels above one default
// batch: 4608-row Q panels at world size > 1 stay one batch, kept in registers)
template <int R, int KU = 0>
__global__ __launch_bounds__(CholNT<R>::value) void k_orth_chol(OrthArgs a) {
    constexpr int NT = CholNT<R>::value;
    __shared__ double redd[NT / 64 * (R * (R + 1) / 2)];
    __shared__ float red[NT / 64 * R];
    __shared__ float tau[(R + 3) / 4 * 4];
    PSGD_STAMP(9);
    __shared__ double gpart[kGramLds<R> ? NT * (R * (R + 1) / 2) : 1];
    __shared__ float top_sh[R * R];
    const OrthUnit u = a.units[blockIdx.x];
    PSGD_STAMP(10);
    if (u.r == 1)  // rank-1 group of a mixed-rank plan: the reference's joint norm, not QR
        orth_joint_norm<NT>(a, u, redd);
    else if (u.r == R)
        orth_chol_panel<R, R, KU>(a, u, redd, red, tau, gpart, top_sh);
    else
        orth_chol_panel<R, 0, KU>(a, u, redd, red, tau, gpart, top_sh);
    PSGD_STAMP(14);
}

// ------------------------------------------- Cholesky-QR for ranks 9-16 on fp64 MFMA ----
// Same algorithm and LAPACK sign reconstruction as k_orth_chol, restructured for a 16-column
// panel, where per-thread r x r register arrays no longer fit:
//  * Gram G = X^T X with v_mfma_f64_16x16x4_f64: a wave loads 4 rows x 16 columns (lane
//    l = X[row0 + l/16][l%16]); that one value is both the A operand (A[i][kk] = X[kk][i])
//    and the B operand (B[kk][j] = X[kk][j]), so each row is read once and the matrix core
//    forms all 256 products. 16 waves accumulate their own rows; partials summed via LDS in
//    a fixed order (bitwise reproducible).
//  * The 16 x 16 chain (Cholesky, R^-1, the signs' LU recursion on the top block) runs on
//    wave 0 with lane-parallel LDS updates.
//  * Y = X M' (M' = R^-1 D) again on the matrix core, transposed: D[c'][rr] = sum M'[l][c]
//    X[row0+rr][l] with a column permutation c = pi(c'); lane l loads X[row0 + l%16][4(l/16)
//    .. +3] (one 16-B load) and writes Y[row0 + l%16][4(l/16) .. +3].
//  * v_mfma_f64_16x16x4_f64 layouts (cdna_hip_programming.md): A[i][k] in lane i + 16k,
//    B[k][j] in lane j + 16k, D[i][j] in lane j + 16 (i % 4), item i / 4.
// Columns >= r (a narrower matrix in the rank-16 bucket) are zero in X and identity in the
// padded Gram, so they do not disturb the first r columns.
typedef double f64x4_t __attribute__((ext_vector_type(4)));
constexpr int kC16NT = 512;
constexpr int kC16W = kC16NT / 64;

__device__ __forceinline__ void lds_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// R = 16 or 32: NB = R / 16 column blocks of 16; the Gram is NB (NB + 1) / 2 MFMA blocks
// (upper), the apply NB x NB blocks of four MFMAs.
template <int R>
__device__ __forceinline__ void orth_chol_wide(const OrthArgs& a) {
    constexpr int NB = R / 16;
    constexpr int NBLK = NB * (NB + 1) / 2;
    constexpr int RR = R * R;
    constexpr int PER = RR / 64;  // r x r entries per lane of wave 0
    // per-wave Gram partials; after the wave sum the same storage holds M', T and X's top block
    constexpr int kScratch = (kC16W * NBLK * 256 > 3 * RR) ? kC16W * NBLK * 256 : 3 * RR;
    __shared__ double scratch[kScratch];
    __shared__ double wsh[RR];  // G, then R (upper, row-major)
    __shared__ double gdiag[R];
    __shared__ double rd[kC16W];
    __shared__ float red[kC16W * R];
    __shared__ float tau[R];
    __shared__ int ok_sh;
    double* gsh = scratch;
    double* msh = scratch;           // M' = R^-1 D (row-major M'[l][c])
    double* tsh = scratch + RR;      // top block T = X[0:r] R^-1
    double* xsh = scratch + 2 * RR;  // top block of X
    const OrthUnit u = a.units[blockIdx.x];
    if (u.r == 1) {  // rank-1 group of a mixed-rank plan: the reference's joint norm
        orth_joint_norm<kC16NT>(a, u, rd);
        return;
    }
    const int r = u.r;
    const int64_t k = u.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ri = lane & 15, kq = lane >> 4;
    float* __restrict__ st = a.state + u.off;
    float* __restrict__ hx = a.hx + u.off;
    float* __restrict__ sv = a.save ? a.save + u.off : nullptr;

    // ---- Gram: wave w takes row quads w, w + 16, ...; kG quads per batch, loads in flight
    constexpr int kG = NB == 1 ? 12 : 6;
    f64x4_t g[NBLK];
#pragma unroll
    for (int bl = 0; bl < NBLK; ++bl) g[bl] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    const int64_t nq = (k + 3) >> 2;
    for (int64_t q0 = wave; q0 < nq; q0 += int64_t(kG) * kC16W) {
        float v[kG][NB];
#pragma unroll
        for (int q = 0; q < kG; ++q) {
            const int64_t row = (q0 + int64_t(q) * kC16W) * 4 + kq;
#pragma unroll
            for (int cb = 0; cb < NB; ++cb) {
                const int c = 16 * cb + ri;
                v[q][cb] = st[(row < k ? row : 0) * r + (c < r ? c : 0)];
            }
        }
#pragma unroll
        for (int q = 0; q < kG; ++q) {
            const int64_t row = (q0 + int64_t(q) * kC16W) * 4 + kq;
#pragma unroll
            for (int cb = 0; cb < NB; ++cb) {
                keep(v[q][cb]);
                const int c = 16 * cb + ri;
                const bool ok = c < r && row < k;
                v[q][cb] = ok ? v[q][cb] : 0.f;
                if (sv && ok) sv[row * r + c] = v[q][cb];
            }
            int bl = 0;
#pragma unroll
            for (int ca = 0; ca < NB; ++ca)
#pragma unroll
                for (int cb = ca; cb < NB; ++cb) {
                    g[bl] = __builtin_amdgcn_mfma_f64_16x16x4f64(double(v[q][ca]), double(v[q][cb]), g[bl], 0, 0, 0);
                    ++bl;
                }
        }
    }
#pragma unroll
    for (int bl = 0; bl < NBLK; ++bl)
#pragma unroll
        for (int e = 0; e < 4; ++e) gsh[(wave * NBLK + bl) * 256 + e * 64 + lane] = g[bl][e];
    __syncthreads();
    for (int t = tid; t < NBLK * 256; t += kC16NT) {  // fixed-order wave sum; f64 D layout
        const int bl = t >> 8, el = t & 255;
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kC16W; ++w) s += gsh[(w * NBLK + bl) * 256 + el];
        int ca = 0, cb = 0, x = bl;  // block index -> (ca <= cb)
        while (x >= NB - ca) { x -= NB - ca; ++ca; }
        cb = ca + x;
        const int e = el >> 6, l = el & 63;
        const int i = 16 * ca + (l >> 4) + 4 * e, j = 16 * cb + (l & 15);
        if (i >= r || j >= r) s = (i == j) ? 1.0 : 0.0;  // identity padding
        wsh[i * R + j] = s;
        if (i == j) gdiag[i] = s;
    }
    __syncthreads();  // gsh is dead from here on (msh / tsh / xsh reuse it)

    if (wave == 0) {
        // top block of X (rows 0..r-1), in flight during the factorisation
        float xt[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = lane + 64 * q, i = e / R, l = e % R;
            xt[q] = st[(i < r ? i : 0) * r + (l < r ? l : 0)];
        }
        // Cholesky G = R^T R (upper R in place), lane-parallel trailing updates
        bool ok = true;
        for (int j = 0; j < R; ++j) {
            lds_fence();
            const double piv = wsh[j * R + j];
            ok = ok && (j >= r || (piv > 1e-8 * gdiag[j] && piv > 0.0));
            const double d = sqrt(piv > 0.0 ? piv : 1.0);
            lds_fence();
            if (lane < R && lane > j) wsh[j * R + lane] = wsh[j * R + lane] / d;
            if (lane == j) wsh[j * R + j] = d;
            lds_fence();
#pragma unroll 4
            for (int q = 0; q < PER; ++q) {
                const int e = lane + 64 * q, i = e / R, b = e % R;
                if (i > j && b >= i) wsh[e] = wsh[e] - wsh[j * R + i] * wsh[j * R + b];
            }
        }
        lds_fence();
        // M = R^-1: lane c owns column c (back substitution; the column lives in LDS, where
        // only lane c touches it, so no register array of R doubles is needed)
        if (lane < R) {
            const int c = lane;
            for (int i = R - 1; i >= 0; --i) {
                double v = (i == c) ? 1.0 : 0.0;
                for (int l = i + 1; l < R; ++l) v -= wsh[i * R + l] * msh[l * R + c];
                msh[i * R + c] = v / wsh[i * R + i];
            }
            for (int i = 0; i < R; ++i)
                if (i >= r || c >= r) msh[i * R + c] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            keep(xt[q]);
            const int e = lane + 64 * q, i = e / R, l = e % R;
            xsh[e] = (i < r && l < r) ? double(xt[q]) : 0.0;
        }
        lds_fence();
        // T = X[0:r] M
#pragma unroll 1
        for (int q = 0; q < PER; ++q) {
            const int e = lane + 64 * q, i = e / R, c = e % R;
            double v = 0.0;
#pragma unroll 16
            for (int l = 0; l < R; ++l) v += xsh[i * R + l] * msh[l * R + c];
            tsh[e] = v;
        }
        // LAPACK's column signs: the LU recursion of k_orth_chol, lane-parallel
        double sg = 1.0;  // lane c < r ends with sgn[c]
        for (int j = 0; j < r; ++j) {
            lds_fence();
            const double tjj = tsh[j * R + j];
            const bool nonneg = tjj >= 0.0;
            ok = ok && !(j < k - 1 && fabs(tjj) > 1.0 - kSignTol);  // see orth_chol_panel
            const double sj = (j == k - 1) ? (nonneg ? 1.0 : -1.0) : (nonneg ? -1.0 : 1.0);
            if (lane == j) sg = sj;
            const double piv = tjj - sj;
#pragma unroll 4
            for (int q = 0; q < PER; ++q) {
                const int e = lane + 64 * q, i = e / R, b = e % R;
                if (i > j && i < r && b > j && b < r) tsh[e] = tsh[e] - (tsh[i * R + j] / piv) * tsh[j * R + b];
            }
        }
        lds_fence();
        if (lane < R) {
#pragma unroll
            for (int i = 0; i < R; ++i) msh[i * R + lane] = msh[i * R + lane] * sg;
        }
        if (lane == 0) ok_sh = ok ? 1 : 0;
    }
    __syncthreads();
    if (!ok_sh && !(a.flags & 1)) {  // exact Householder (geqr2 + org2r) in place in hx
        for (int64_t i = tid; i < k * r; i += kC16NT) hx[i] = st[i];
        __syncthreads();
        householder_q<R, kC16NT>(hx, k, r, red, tau);
        for (int64_t i = tid; i < k * r; i += kC16NT) st[i] = hx[i];
        return;
    }

    // ---- Y = X M' on the matrix core: 16-row blocks, wave w takes blocks w, w + 16, ...
    // Output block cb, inner block lb, MFMA e covers inner columns l = 16 lb + 4 kk + e:
    // A[i = ri][kk = kq] = M'[16 lb + 4 kq + e][16 cb + pi(ri)], pi(i) = 4 (i & 3) + (i >> 2):
    // the f64 D layout puts row (l>>4) + 4e in lane l, item e, so this output-column
    // permutation hands lane l the four contiguous columns 16 cb + 4 kq .. + 3 of its row
    double am[NB][NB][4];
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
        for (int lb = 0; lb < NB; ++lb)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                am[cb][lb][e] = msh[(16 * lb + 4 * kq + e) * R + 16 * cb + 4 * (ri & 3) + (ri >> 2)];
    __syncthreads();  // the top block was read (wave 0) before any row is overwritten
    constexpr int kA = NB == 1 ? 6 : 3;
    const int64_t nb = (k + 15) >> 4;
    // 16-B rows: one load per lane per block and column block (state offsets of a
    // mixed-rank plan need not be multiples of 4 floats)
    const bool vec = r == R && ((reinterpret_cast<uintptr_t>(st) | reinterpret_cast<uintptr_t>(hx)) & 15) == 0;
    for (int64_t b0 = wave; b0 < nb; b0 += int64_t(kA) * kC16W) {
        float x[kA][NB][4];
#pragma unroll
        for (int q = 0; q < kA; ++q) {
            const int64_t row = (b0 + int64_t(q) * kC16W) * 16 + ri;
            const int64_t rc = row < k ? row : 0;
#pragma unroll
            for (int lb = 0; lb < NB; ++lb) {
                if (vec) {
                    const float4 t = *reinterpret_cast<const float4*>(st + rc * R + 16 * lb + 4 * kq);
                    x[q][lb][0] = t.x; x[q][lb][1] = t.y; x[q][lb][2] = t.z; x[q][lb][3] = t.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = 16 * lb + 4 * kq + e;
                        x[q][lb][e] = st[rc * r + (c < r ? c : 0)];
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kA; ++q) {
            const int64_t row = (b0 + int64_t(q) * kC16W) * 16 + ri;
#pragma unroll
            for (int lb = 0; lb < NB; ++lb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    keep(x[q][lb][e]);
                    x[q][lb][e] = (16 * lb + 4 * kq + e < r) ? x[q][lb][e] : 0.f;
                }
#pragma unroll
            for (int cb = 0; cb < NB; ++cb) {
                f64x4_t y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int lb = 0; lb < NB; ++lb)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        y = __builtin_amdgcn_mfma_f64_16x16x4f64(am[cb][lb][e], double(x[q][lb][e]), y, 0, 0, 0);
                // lane l holds D[kq + 4e][ri] = Y[row0 + ri][16 cb + pi(kq + 4e) = 16 cb + 4 kq + e]
                if (row < k) {
                    if (vec) {
                        const float4 o = make_float4(float(y[0]), float(y[1]), float(y[2]), float(y[3]));
                        *reinterpret_cast<float4*>(st + row * R + 16 * cb + 4 * kq) = o;
                        *reinterpret_cast<float4*>(hx + row * R + 16 * cb + 4 * kq) = o;
                    } else {
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
    }
}

__global__ __launch_bounds__(kC16NT) void k_orth_chol16(OrthArgs a) { orth_chol_wide<16>(a); }
__global__ __launch_bounds__(kC16NT) void k_orth_chol32(OrthArgs a) { orth_chol_wide<32>(a); }

// ------------------------------------------- folded Cholesky-QR (projection form) ----
// The Q panels of a two-iteration rank-2/4 step at world size 1: k_reduce left each item's
// upper Gram (fp64) beside the reduced factor, so no pass over the panel forms it. Workgroup
// (unit, slice) sums its unit's item partials (lane-strided in item order, then the wave
// tree: fixed order, the same in every slice), runs k_orth_chol's chain (Cholesky, R^-1,
// LAPACK signs from the top rows) and writes X = raw M D for its kChainRows rows (the same
// fp64 row products as k_orth_chol's second pass): the panel is read once, spread over
// ceil(k / kChainRows) CUs instead of one. A panel the chain rejects takes the exact
// Householder recursion in slice 0 (the other slices return).
// rows per thread of k_orth_chain: 1 (one 512-row slice per workgroup; cfg3 0.0911-0.0912 ->
// 0.0908 ms against 2, 4 slower: 0.0914-0.0915, profiles/r05/orth/r05ar_chain_rows.txt)
#ifndef PSGD_CHAIN_NT
#define PSGD_CHAIN_NT 512
#endif
#ifndef PSGD_CHAIN_ROWS
#define PSGD_CHAIN_ROWS 1
#endif
template <int R>
__global__ __launch_bounds__(PSGD_CHAIN_NT) void k_orth_chain(ChainArgs a) {
    constexpr int NT = PSGD_CHAIN_NT;
    constexpr int NG = R * (R + 1) / 2;
    constexpr int kRows = PSGD_CHAIN_ROWS;  // rows per thread: kChainRows = kRows NT
    __shared__ double m_sh[R * R];
    __shared__ int ok_sh;
    __shared__ float top_sh[R * R];
    __shared__ float red[NT / 64 * R];
    __shared__ float tau[(R + 3) / 4 * 4];
    const OrthUnit u = a.units[blockIdx.x];
    const int r = R;  // the plan folds only panels of exactly R columns
    const int64_t k = u.k;
    const int64_t row0 = int64_t(blockIdx.y) * kRows * NT;
    if (row0 >= k) return;  // uniform: short panels use fewer slices
    const int tid = threadIdx.x, lane = tid & 63;
    const float* raw = a.raw + u.off;
    // this slice's rows go out first (in flight during the partial sums and the chain)
    float x[kRows][R];
#pragma unroll
    for (int q = 0; q < kRows; ++q) {
        const int64_t i = row0 + tid + int64_t(q) * NT;
        ld_row<R>(raw + (i < k ? i : 0) * r, r, x[q]);
    }
    if (tid < R * R) top_sh[tid] = raw[tid];  // the top R rows (k >= r)
    double g[NG];
    if (tid < 64) {
        const int ib = a.uitems[2 * blockIdx.x], ie = a.uitems[2 * blockIdx.x + 1];
#pragma unroll
        for (int e = 0; e < NG; ++e) g[e] = 0.0;
        for (int it0 = ib + lane; it0 < ie; it0 += 64) {
#pragma unroll
            for (int e = 0; e < NG; ++e) g[e] += a.gram[int64_t(it0) * kGramStride + e];
        }
#pragma unroll
        for (int e = 0; e < NG; ++e) g[e] = wave_allsum_f64(g[e]);
    }
    __syncthreads();  // top_sh
    if (tid < 64) chol_chain<R>(g, top_sh, raw, r, k, m_sh, &ok_sh, blockIdx.y == 0 ? a.rfac + u.off : nullptr);
    __syncthreads();
    float* st = a.state + u.off;
    float* hx = a.hx + u.off;
    if (!ok_sh) {
        if (blockIdx.y != 0) return;
        // exact Householder (geqr2 + org2r) in the history buffer, then the state
        for (int64_t i = tid; i < k * r; i += NT) hx[i] = raw[i];
        __syncthreads();
        householder_q<R, NT>(hx, k, r, red, tau, a.rfac + u.off);
        for (int64_t i = tid; i < k * r; i += NT) st[i] = hx[i];
        return;
    }
    double M[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int c = 0; c < R; ++c) M[i][c] = m_sh[i * R + c];
#pragma unroll
    for (int q = 0; q < kRows; ++q) {
        const int64_t i = row0 + tid + int64_t(q) * NT;
#pragma unroll
        for (int c = 0; c < R; ++c) keep(x[q][c]);
        float y[R];
#pragma unroll
        for (int c = 0; c < R; ++c) {
            double v = 0.0;
#pragma unroll
            for (int l = 0; l < R; ++l) v += double(x[q][l]) * M[l][c];
            y[c] = float(v);
        }
        if (i < k) {
            st_row<R>(st + i * r, r, y);
            st_row<R>(hx + i * r, r, y);
        }
    }
}

// rank 4, panels longer than one default batch (8 x 512 rows) up to 10 x 512: the 10-row
// batch instance (W > 1 Q panels of ResNet-50: k_orth_chol<4> ~1 us faster; on the <= 4096-row
// P panels the default batch stays faster, profiles/r05/orth)
#ifndef PSGD_CHOL_U4L
#define PSGD_CHOL_U4L 10
#endif
constexpr int kCholKU4Long = PSGD_CHOL_U4L > PSGD_CHOL_U4 ? PSGD_CHOL_U4L : PSGD_CHOL_U4 + 1;
// rank 4, panels of at most 4 x 512 rows (ResNet-50's P panels): 4-row batches, no clamped loads
#ifndef PSGD_CHOL_U4S
#define PSGD_CHOL_U4S 4
#endif
constexpr int kCholKU4Short = PSGD_CHOL_U4S > 0 ? PSGD_CHOL_U4S : 1;
// rank 2, panels up to 22 x 512 rows (LLaMA's 11008-row Q panels) in one register-resident batch
#ifndef PSGD_CHOL_U2L
#define PSGD_CHOL_U2L 22
#endif
constexpr int kCholKU2Long = PSGD_CHOL_U2L > PSGD_CHOL_U2 ? PSGD_CHOL_U2L : PSGD_CHOL_U2 + 1;
inline hipError_t launch_orth_chol(const OrthArgs& a, int nunits, int R, int64_t kmax, hipStream_t s) {
    switch (R) {
        case 2:
            if (PSGD_CHOL_U2L > PSGD_CHOL_U2 && kmax > int64_t(PSGD_CHOL_U2) * CholNT<2>::value && kmax <= int64_t(kCholKU2Long) * CholNT<2>::value)
                k_orth_chol<2, kCholKU2Long><<<nunits, CholNT<2>::value, 0, s>>>(a);
            else
                k_orth_chol<2><<<nunits, CholNT<2>::value, 0, s>>>(a);
            break;
        case 4:
            if (PSGD_CHOL_U4S > 0 && PSGD_CHOL_U4S < PSGD_CHOL_U4 && kmax <= int64_t(kCholKU4Short) * CholNT<4>::value)
                k_orth_chol<4, kCholKU4Short><<<nunits, CholNT<4>::value, 0, s>>>(a);
            else if (PSGD_CHOL_U4L > PSGD_CHOL_U4 && kmax > int64_t(PSGD_CHOL_U4) * CholNT<4>::value && kmax <= int64_t(kCholKU4Long) * CholNT<4>::value)
                k_orth_chol<4, kCholKU4Long><<<nunits, CholNT<4>::value, 0, s>>>(a);
            else
                k_orth_chol<4><<<nunits, CholNT<4>::value, 0, s>>>(a);
            break;
        case 8: k_orth_chol<8><<<nunits, CholNT<8>::value, 0, s>>>(a); break;
        case 16: k_orth_chol16<<<nunits, kC16NT, 0, s>>>(a); break;
        case 32: k_orth_chol32<<<nunits, kC16NT, 0, s>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace psgd
