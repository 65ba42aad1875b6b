// Kernels of psgd_clip_outputs (psgd_norm.h): the global L2 norm of a step's averages from the
// low-rank factors (k_norm_gram, k_norm_mat) or from the dense outputs (k_norm_stream), the
// finishing step (k_norm_finish: norm and clip coefficient, device-side) and the scale pass
// (k_norm_scale; k_norm_scale_dst of psgd_clip_dst: through per-tensor destination tables), which
// exits at once when nothing is clipped.
//
// Codegen rules as everywhere in the codec: global pointers in address space
// 1 or buffer descriptors, unconditional loads from clamped addresses masked by selects, every
// reduction in a fixed order with no float atomics (results are bitwise reproducible), no scratch.
// All accumulation is fp64: a product of two fp32 values is exact in fp64, so the only rounding is
// the running sum's.
#include <hip/hip_runtime.h>

#include "psgd_norm.h"
#include "psgd_stream.cuh"

namespace psgd {

namespace {

// fixed-order sum over the workgroup's kBlock threads: an xor tree inside each wave, then the
// waves in order; the result is valid in every thread
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();  // `sh` may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double t = sh[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) t += sh[k];
    return t;
}

// entry e of the row-major upper triangle of a K x K matrix -> (a, b), a <= b
__device__ __forceinline__ void tri_decode(int e, int K, int& a, int& b) {
    a = 0;
    int rem = e, len = K;
    while (rem >= len) {
        rem -= len;
        --len;
        ++a;
    }
    b = a + rem;
}

}  // namespace

// ---------------------------------------------------------------- stream form
template <typename T>
struct NormIo;
template <>
struct NormIo<float> {
    static constexpr int V = 4;
    typedef v4f vec;
    static __device__ __forceinline__ double sq(const vec& x) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < V; ++e) s = fma(double(x[e]), double(x[e]), s);
        return s;
    }
    static __device__ __forceinline__ double sq1(float x) { return double(x) * double(x); }
    static __device__ __forceinline__ float scale1(float x, float c32, double) { return x * c32; }
    static __device__ __forceinline__ vec scale(const vec& x, float c32, double) { return x * c32; }
};
template <>
struct NormIo<bf16_t> {
    static constexpr int V = 8;
    typedef unsigned vec __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ double sq(const vec& x) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double lo = double(__uint_as_float(x[e] << 16)), hi = double(__uint_as_float(x[e] & 0xffff0000u));
            s = fma(lo, lo, s);
            s = fma(hi, hi, s);
        }
        return s;
    }
    static __device__ __forceinline__ double sq1(bf16_t x) { return double(bf2f(x)) * double(bf2f(x)); }
    static __device__ __forceinline__ bf16_t scale1(bf16_t x, float c32, double) { return f2bf(bf2f(x) * c32); }
    static __device__ __forceinline__ vec scale(const vec& x, float c32, double) {
        vec y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(x[e] << 16) * c32, hi = __uint_as_float(x[e] & 0xffff0000u) * c32;
            y[e] = uint32_t(f2bf(lo)) | (uint32_t(f2bf(hi)) << 16);
        }
        return y;
    }
};
template <>
struct NormIo<double> {
    static constexpr int V = 2;
    typedef double vec __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ double sq(const vec& x) { return fma(x[1], x[1], x[0] * x[0]); }
    static __device__ __forceinline__ double sq1(double x) { return x * x; }
    static __device__ __forceinline__ double scale1(double x, float, double c) { return x * c; }
    static __device__ __forceinline__ vec scale(const vec& x, float, double c) { return x * c; }
};

// A dense range of n elements at `p` as [head | 16-byte vectors | tail]: the head runs to the
// first 16-byte boundary (fewer than V elements), the tail holds what no whole vector covers
template <typename T>
struct NormSplit {
    int64_t head, nvec, tail;
    __device__ __forceinline__ NormSplit(const T* p, int64_t n) {
        constexpr int V = NormIo<T>::V;
        const int64_t mis = int64_t((reinterpret_cast<uintptr_t>(p) & 15) / sizeof(T));
        head = mis ? V - mis : 0;
        if (head > n) head = n;
        nvec = (n - head) / V;
        tail = n - head - nvec * V;
    }
};

// Workgroup `blk` of the two ranges' nwg[0] + nwg[1]: vectors [w * per, (w + 1) * per) of its
// range's body, workgroup 0 of a range also the scalar head and tail. One partial per workgroup
// (part_[blk]), summed in a fixed order.
template <typename T>
__device__ __forceinline__ void norm_stream_block(const NormRangeArgs& r, int blk, double* part_, double* sh) {
    using Io = NormIo<T>;
    typedef typename Io::vec vec;
    const int which = blk < r.nwg[0] ? 0 : 1;
    const int w = blk - (which ? r.nwg[0] : 0);
    const T* p = static_cast<const T*>(r.base[which]);
    const int64_t n = r.numel[which];
    const NormSplit<T> sp(p, n);
    const int64_t per = (sp.nvec + r.nwg[which] - 1) / r.nwg[which];
    const int64_t lo = int64_t(w) * per, hi = lo + per < sp.nvec ? lo + per : sp.nvec;
    const gptr<const vec> body = (gptr<const vec>)(reinterpret_cast<const vec*>(p + sp.head));
    const gptr<const T> el = gconst<T>(p);
    double acc = 0.0;
    for (int64_t b = lo; b < hi; b += 4 * kBlock) {
        vec x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = b + u * kBlock + threadIdx.x;
            x[u] = body[i < hi ? i : hi - 1];  // clamped, unconditional
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = b + u * kBlock + threadIdx.x;
            const double s = Io::sq(x[u]);
            acc += i < hi ? s : 0.0;
        }
    }
    if (w == 0) {  // head and tail: fewer than 2 V elements, one per thread
        const int64_t ns = sp.head + sp.tail, t = threadIdx.x;
        const int64_t i = t < sp.head ? t : n - sp.tail + (t - sp.head);
        const T x = el[t < ns ? i : 0];
        const double s = Io::sq1(x);
        acc += t < ns ? s : 0.0;
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) gmut<double>(part_)[blk] = t;
}
// dtype: 0 fp32, 1 bf16, 2 fp64 (psgd_dtype, include/psgd.h); workgroup-uniform
__device__ __forceinline__ void norm_stream_any(int dtype, const NormRangeArgs& r, int blk, double* part_, double* sh) {
    if (dtype == 0)
        norm_stream_block<float>(r, blk, part_, sh);
    else if (dtype == 1)
        norm_stream_block<bf16_t>(r, blk, part_, sh);
    else
        norm_stream_block<double>(r, blk, part_, sh);
}

// ---------------------------------------------------------------- factor form
// One workgroup per NormItem: the upper triangle of sum_rows x x^T over the item's rows of the
// stacked factor x = [term 0 | .. | term I-1] (K = I * r columns). kNormChunk rows at a time are
// staged in LDS (each term's rows are contiguous in its panel: coalesced loads); thread t owns
// entries t, t + 256, .. (EPT of them, in registers). Narrow stacks (at most 128 entries) split the
// staged rows over 256 / NEP thread groups, whose sums are added in group order at the end.
// A pass stages as many rows as the LDS image holds at this K (kNormChunk at K = 64, a whole
// 256-row item up to K = 8: one batch of loads per item, no dependent chain of chunks).
// Workgroups nitems .. nitems + rg.nwg[0] + rg.nwg[1] - 1 are stream-form workgroups over the dense
// ranges `rg` (the uncompressed slab) in the same launch.
template <int EPT>
__global__ __launch_bounds__(kBlock) void k_norm_gram(NormGramArgs a, int nitems, NormRangeArgs rg, double* spart,
                                                     int dtype) {
    __shared__ __attribute__((aligned(16))) float xs[kNormChunk * kNormMaxK];
    __shared__ double red[kBlock];
    if (int(blockIdx.x) >= nitems) {
        norm_stream_any(dtype, rg, int(blockIdx.x) - nitems, spart, red);
        return;
    }
    const NormItem it = a.items[blockIdx.x];
    const MatDesc d = a.mats[it.mat];
    const int r = d.r, K = a.nterms * r, ne = K * (K + 1) / 2;
    const int tid = threadIdx.x;
    const int64_t base = (it.side ? d.qoff : d.poff) + int64_t(it.row0) * r;
    int nep = kBlock;  // threads per row group
    if (EPT == 1 && ne <= kBlock / 2) {
        nep = 1;
        while (nep < ne) nep <<= 1;
    }
    const int nsub = kBlock / nep, sub = tid / nep, e0 = tid - sub * nep;
    int ea[EPT], eb[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = e0 + j * kBlock;
        tri_decode(e < ne ? e : 0, K, ea[j], eb[j]);
    }
    double acc[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) acc[j] = 0.0;

    const int chunk = kNormChunk * kNormMaxK / K;  // rows per pass: >= kNormChunk, K * chunk floats fit xs
    for (int c0 = 0; c0 < it.rows; c0 += chunk) {
        const int crow = it.rows - c0 < chunk ? it.rows - c0 : chunk;
        const int cnt = crow * r;  // contiguous floats of this chunk in every term's panel
        __syncthreads();           // the previous chunk's reads are done
        for (int k = 0; k < a.nterms; ++k) {
            const gptr<const float> src = gconst<float>(it.side ? a.apx.q[k] : a.apx.p[k]) + base + int64_t(c0) * r;
            for (int i = tid; i < cnt; i += kBlock) {
                const int rr = i / r;
                xs[rr * K + k * r + (i - rr * r)] = src[i];
            }
        }
        __syncthreads();
        for (int rr = sub; rr < crow; rr += nsub) {
            const float* x = xs + rr * K;
#pragma unroll
            for (int j = 0; j < EPT; ++j) acc[j] = fma(double(x[ea[j]]), double(x[eb[j]]), acc[j]);
        }
    }
    const gptr<double> out = gmut<double>(a.part) + it.part;
    if constexpr (EPT == 1) {
        if (nsub > 1) {  // the row groups' sums, in group order
            red[tid] = acc[0];
            __syncthreads();
            if (sub == 0 && e0 < ne) {
                double t = red[e0];
                for (int g = 1; g < nsub; ++g) t += red[e0 + g * nep];
                out[e0] = t;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = e0 + j * kBlock;
        if (e < ne) out[e] = acc[j];
    }
}

// One workgroup per matrix: the items' partials of each side summed in item (row) order, then
// alpha^2 sum_{a <= b} w G_P[a, b] G_Q[a, b], w = 1 on the diagonal and 2 off it.
__global__ __launch_bounds__(kBlock) void k_norm_mat(NormMatArgs a) {
    __shared__ double sh[kWaves];
    const MatDesc d = a.mats[blockIdx.x];
    const NormMat nm = a.nmats[blockIdx.x];
    const int K = a.nterms * d.r, ne = K * (K + 1) / 2;
    const gptr<const double> part = gconst<double>(a.part);
    const int64_t p0 = a.items[nm.item0[0]].part, q0 = a.items[nm.item0[1]].part;
    double loc = 0.0;
    for (int e = threadIdx.x; e < ne; e += kBlock) {
        double gp = 0.0, gq = 0.0;
        for (int i = 0; i < nm.nitems[0]; ++i) gp += part[p0 + int64_t(i) * ne + e];
        for (int i = 0; i < nm.nitems[1]; ++i) gq += part[q0 + int64_t(i) * ne + e];
        int ra, rb;
        tri_decode(e, K, ra, rb);
#ifdef PSGD_NORM_DROP_CROSS  // diagnostic builds only: the blocks between different iterations left out
        if (ra / d.r != rb / d.r) gp = 0.0;
#endif
        loc += (ra == rb ? 1.0 : 2.0) * gp * gq;
    }
    const double t = block_sum(loc, sh);
    if (threadIdx.x == 0) gmut<double>(a.sq)[d.tensor] = a.alpha * a.alpha * t;
}

// ---------------------------------------------------------------- stream form (a launch of its own)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_norm_stream(NormRangeArgs r, double* part_) {
    __shared__ double sh[kWaves];
    norm_stream_block<T>(r, int(blockIdx.x), part_, sh);
}

// ---------------------------------------------------------------- finish
// One workgroup. sq_compressed: the per-tensor squares added in tensor order (factor form), or
// range 0's partials; sq_flat: range 1's partials. Partials are summed thread-strided, then by the
// fixed tree. norm = sqrt(sq_compressed + sq_flat); coef = min(1, max_norm / (norm + 1e-6)) as
// torch.nn.utils.clip_grad_norm_; a non-finite norm gives coef = NaN (nothing is scaled).
__global__ __launch_bounds__(kBlock) void k_norm_finish(NormFinishArgs a) {
    __shared__ double sh[kWaves];
    const gptr<const double> part = gconst<double>(a.part);
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < a.npart[0]; i += kBlock) s0 += part[i];
    for (int i = threadIdx.x; i < a.npart[1]; i += kBlock) s1 += part[a.npart[0] + i];
    double sqc = block_sum(s0, sh);
    const double sqf = block_sum(s1, sh);
    if (threadIdx.x != 0) return;
    if (a.sq) {
        const gptr<const double> sq = gconst<double>(a.sq);
        sqc = 0.0;
        for (int i = 0; i < a.nsq; ++i) sqc += sq[i];
    }
    const double norm = sqrt(sqc + sqf);
    double coef = a.max_norm / (norm + 1e-6);
    coef = coef < 1.0 ? coef : 1.0;
    if (!isfinite(norm)) coef = __builtin_nan("");
    const gptr<double> res = gmut<double>(a.result);
    res[0] = norm;
    res[1] = coef;
}

// ---------------------------------------------------------------- scale
// x <- x * coef over both ranges, kNormVecs vectors per workgroup; a workgroup returns at once,
// writing nothing, unless coef < 1 and the norm is finite. Stores stream write-through like the
// final passes' (PSGD_ST_AUX), through a descriptor that spans the workgroup's own vectors.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_norm_scale(NormRangeArgs r, const double* result) {
    using Io = NormIo<T>;
    typedef typename Io::vec vec;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const gptr<const double> res = gconst<double>(result);
    const double norm = res[0], coef = res[1];
    if (!(coef < 1.0) || !isfinite(norm)) return;
    const float c32 = float(coef);
    const int which = int(blockIdx.x) < r.nwg[0] ? 0 : 1;
    const int w = int(blockIdx.x) - (which ? r.nwg[0] : 0);
    T* p = static_cast<T*>(r.base[which]);
    const int64_t n = r.numel[which];
    const NormSplit<T> sp(p, n);
    const int64_t lo = int64_t(w) * kNormVecs, hi = lo + kNormVecs < sp.nvec ? lo + kNormVecs : sp.nvec;
    if (hi > lo) {
        const vec* vb = reinterpret_cast<const vec*>(p + sp.head) + lo;
        const gptr<const vec> body = (gptr<const vec>)(vb);
        const rsrc_t rs = make_rsrc(vb, uint32_t(hi - lo) * 16u);
        constexpr int PER = kNormVecs / kBlock;
        const int cnt = int(hi - lo);
#pragma unroll 4
        for (int q = 0; q < PER; ++q) {
            const int i = q * kBlock + int(threadIdx.x);
            const vec x = body[i < cnt ? i : cnt - 1];  // clamped, unconditional
            const vec y = Io::scale(x, c32, coef);
            if (i < cnt) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, y), rs, uint32_t(i) * 16u, 0, PSGD_ST_AUX);
        }
    }
    if (w == 0) {
        const int64_t ns = sp.head + sp.tail, t = threadIdx.x;
        if (t < ns) {
            const int64_t i = t < sp.head ? t : n - sp.tail + (t - sp.head);
            const rsrc_t re = make_rsrc(p + i, uint32_t(sizeof(T)));
            const T y = Io::scale1(gconst<T>(p)[i], c32, coef);
            if constexpr (sizeof(T) == 2)
                __builtin_amdgcn_raw_buffer_store_b16(y, re, 0, 0, PSGD_ST_AUX);
            else if constexpr (sizeof(T) == 4)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), re, 0, 0, PSGD_ST_AUX);
            else
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, y), re, 0, 0, PSGD_ST_AUX);
        }
    }
}

// ---------------------------------------------------------------- scale, destination tables
// psgd_clip_dst: x <- x * float(coef) through two tables of per-tensor destinations (fp32 views
// inside DDP buckets: 4-byte aligned, no better in general), one NormDstItem per workgroup; the
// same early return as k_norm_scale. The item's pointer decides its split once: a head of 0-3
// elements up to the first 16-byte boundary, 16-byte vectors, a tail of 0-3 elements. Every load
// (kNormDstVecs vectors per thread through a descriptor that spans the item's own vectors, clamped
// offsets; one head / tail element per thread from a clamped address-space-1 address) is issued
// before the first store; vector stores go through the same descriptor, element stores through
// one-element descriptors, both write-through (PSGD_ST_AUX). Nothing outside the item's `cnt`
// elements is read or written.
__global__ __launch_bounds__(kBlock) void k_norm_scale_dst(NormDstArgs a, const double* result) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const gptr<const double> res = gconst<double>(result);
    const double norm = res[0], coef = res[1];
    if (!(coef < 1.0) || !isfinite(norm)) return;
    const float c32 = float(coef);
    const int which = int(blockIdx.x) < a.nitems[0] ? 0 : 1;
    const NormDstItem it = a.items[which][int(blockIdx.x) - (which ? a.nitems[0] : 0)];
    float* p = static_cast<float*>(a.table[which][it.tensor]) + it.off;
    const int mis = int((reinterpret_cast<uintptr_t>(p) & 15) >> 2);
    int head = mis ? 4 - mis : 0;
    if (head > it.cnt) head = it.cnt;
    const int nvec = (it.cnt - head) >> 2, tail = it.cnt - head - 4 * nvec;
    const rsrc_t rv = make_rsrc(p + head, uint32_t(nvec) * 16u);
    const int tid = int(threadIdx.x);
    v4u x[kNormDstVecs];
#pragma unroll
    for (int q = 0; q < kNormDstVecs; ++q) {
        const int i = q * kBlock + tid;
        const int c = i < nvec ? i : nvec > 0 ? nvec - 1 : 0;  // clamped, unconditional (no vectors: reads 0)
        x[q] = __builtin_amdgcn_raw_buffer_load_b128(rv, uint32_t(c) * 16u, 0, 0);
    }
    // head and tail: at most 6 elements, one per thread
    const int ns = head + tail;
    const int ei = tid < head ? tid : it.cnt - tail + (tid - head);
    const float e = gconst<float>(p)[tid < ns ? ei : 0];
#pragma unroll
    for (int q = 0; q < kNormDstVecs; ++q) {
        const int i = q * kBlock + tid;
        const v4f y = __builtin_bit_cast(v4f, x[q]) * c32;
        if (i < nvec) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, y), rv, uint32_t(i) * 16u, 0, PSGD_ST_AUX);
    }
    if (tid < ns) {
        const rsrc_t re = make_rsrc(p + ei, 4u);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(e * c32), re, 0, 0, PSGD_ST_AUX);
    }
}

// ---------------------------------------------------------------- launchers
hipError_t launch_norm_gram(int ept, const NormGramArgs& a, int nitems, int dtype, const NormRangeArgs& rg,
                            double* spart, hipStream_t s) {
    const int n = nitems + rg.nwg[0] + rg.nwg[1];
    if (n == 0) return hipSuccess;
    switch (ept) {
        case 1: k_norm_gram<1><<<n, kBlock, 0, s>>>(a, nitems, rg, spart, dtype); break;
        case 2: k_norm_gram<2><<<n, kBlock, 0, s>>>(a, nitems, rg, spart, dtype); break;
        case 4: k_norm_gram<4><<<n, kBlock, 0, s>>>(a, nitems, rg, spart, dtype); break;
        case 9: k_norm_gram<9><<<n, kBlock, 0, s>>>(a, nitems, rg, spart, dtype); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_norm_mat(const NormMatArgs& a, int nmats, hipStream_t s) {
    if (nmats == 0) return hipSuccess;
    k_norm_mat<<<nmats, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

// dtype: 0 fp32, 1 bf16, 2 fp64 (psgd_dtype, include/psgd.h)
hipError_t launch_norm_stream(int dtype, const NormRangeArgs& r, double* part, hipStream_t s) {
    const int n = r.nwg[0] + r.nwg[1];
    if (n == 0) return hipSuccess;
    if (dtype == 0)
        k_norm_stream<float><<<n, kBlock, 0, s>>>(r, part);
    else if (dtype == 1)
        k_norm_stream<bf16_t><<<n, kBlock, 0, s>>>(r, part);
    else
        k_norm_stream<double><<<n, kBlock, 0, s>>>(r, part);
    return hipGetLastError();
}

hipError_t launch_norm_finish(const NormFinishArgs& a, hipStream_t s) {
    k_norm_finish<<<1, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_norm_scale(int dtype, const NormRangeArgs& r, const double* result, hipStream_t s) {
    const int n = r.nwg[0] + r.nwg[1];
    if (n == 0) return hipSuccess;
    if (dtype == 0)
        k_norm_scale<float><<<n, kBlock, 0, s>>>(r, result);
    else if (dtype == 1)
        k_norm_scale<bf16_t><<<n, kBlock, 0, s>>>(r, result);
    else
        k_norm_scale<double><<<n, kBlock, 0, s>>>(r, result);
    return hipGetLastError();
}

hipError_t launch_norm_scale_dst(const NormDstArgs& a, const double* result, hipStream_t s) {
    const int n = a.nitems[0] + a.nitems[1];
    if (n == 0) return hipSuccess;
    k_norm_scale_dst<<<n, kBlock, 0, s>>>(a, result);
    return hipGetLastError();
}

namespace {
template <typename K>
int kernel_waves(K k) {
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k)) != hipSuccess) return 0;
    if (fa.localSizeBytes != 0) return 0;  // scratch
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, kBlock, 0) != hipSuccess) return 0;
    return blocks * kWaves / 4;  // 4 SIMDs per CU
}
}  // namespace

int norm_min_waves() {
    int w = kernel_waves(k_norm_gram<1>);
    w = std::min(w, kernel_waves(k_norm_gram<2>));
    w = std::min(w, kernel_waves(k_norm_gram<4>));
    w = std::min(w, kernel_waves(k_norm_gram<9>));
    w = std::min(w, kernel_waves(k_norm_mat));
    w = std::min(w, kernel_waves(k_norm_stream<float>));
    w = std::min(w, kernel_waves(k_norm_stream<bf16_t>));
    w = std::min(w, kernel_waves(k_norm_stream<double>));
    w = std::min(w, kernel_waves(k_norm_finish));
    w = std::min(w, kernel_waves(k_norm_scale<float>));
    w = std::min(w, kernel_waves(k_norm_scale<bf16_t>));
    w = std::min(w, kernel_waves(k_norm_scale<double>));
    w = std::min(w, kernel_waves(k_norm_scale_dst));
    return w;
}

}  // namespace psgd
