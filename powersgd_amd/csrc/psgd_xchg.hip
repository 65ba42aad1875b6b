// One-shot all-reduce over IPC-mapped exchange buffers (k_xchg).
#include <hip/hip_runtime.h>

#include "psgd_xchg.cuh"   // the flag / wait protocol and the quad sum, shared with k_xchg_mix
#include "psgd_chain.cuh"  // wave_allsum_f64

namespace psgd {

__global__ __launch_bounds__(kBlock) void k_xchg(XchgArgs a) {
    const int tid = threadIdx.x;
    if (xchg_arrive_and_wait(a)) {
        // an invalid exchange returns NaN sums, never plausible stale ones: the
        // factor (and, on the last iteration, the flat tensors) of this workgroup's share
        const float nan = __builtin_nanf("");
        if (a.items) {
            const RedItem it = a.items[blockIdx.x];
            const MatDesc d = a.mats[it.mat];
            const int64_t e = (a.even ? d.qoff : d.poff) + it.start + tid;
            if (tid < it.cnt) a.dst[e] = a.dst2[e] = nan;
            return;
        }
        const int64_t stride = int64_t(gridDim.x) * kBlock;
        for (int64_t i = int64_t(blockIdx.x) * kBlock + tid; i < a.n + a.nflat; i += stride) {
            if (i < a.n) a.dst[i] = nan;
            else a.flat_dst[i - a.n] = nan;
        }
        return;
    }
    if (a.items) {  // one reduction item per workgroup (<= 256 consecutive factor elements)
        __shared__ float wsq[kWaves];
        __shared__ float xv[kRedItem];
        const RedItem it = a.items[blockIdx.x];
        const MatDesc d = a.mats[it.mat];
        const int64_t e = (a.even ? d.qoff : d.poff) + it.start + tid;
        float sq = 0.f, s = 0.f;
        if (tid < it.cnt) {
            for (int w0 = 0; w0 < a.world; w0 += kXchgUnroll) {  // the peers' loads in flight together
                float v[kXchgUnroll];
#pragma unroll
                for (int u = 0; u < kXchgUnroll; ++u)  // uniform guard: no load past the last peer
                    v[u] = w0 + u < a.world
                               ? __hip_atomic_load(reinterpret_cast<const float*>(a.peers[w0 + u] + a.slot_off) + e,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                               : 0.f;
#pragma unroll
                for (int u = 0; u < kXchgUnroll; ++u)
                    if (w0 + u < a.world) s = w0 + u == 0 ? v[u] : s + v[u];  // rank order
            }
            a.dst[e] = s;
            a.dst2[e] = s;
            sq = s * s;
        }
        if (a.ss_out) {
            sq = wave_allsum(sq);
            if ((tid & 63) == 0) wsq[tid >> 6] = sq;
            __syncthreads();
            if (tid == 0) a.ss_out[blockIdx.x] = ((wsq[0] + wsq[1]) + wsq[2]) + wsq[3];
        }
        if (a.gram) {
            // the item's rows (it starts on a row and holds whole rows of r elements): lane l
            // of wave 0 takes rows l, l + 64, ...; fp64 products, one wave tree per entry
            xv[tid] = s;
            __syncthreads();
            if (tid >= 64) return;
            const int r = a.gram_r, nrow = it.cnt / r;
            double g[kGramStride];
#pragma unroll
            for (int k = 0; k < kGramStride; ++k) g[k] = 0.0;
            for (int row = tid; row < nrow; row += 64) {
                int k = 0;
                for (int c = 0; c < r; ++c)
                    for (int b = c; b < r; ++b) {
                        const double prod = double(xv[row * r + c]) * double(xv[row * r + b]);
#pragma unroll
                        for (int q = 0; q < kGramStride; ++q)
                            if (q == k) g[q] += prod;
                        ++k;
                    }
            }
            const int ng = r * (r + 1) / 2;
#pragma unroll
            for (int k = 0; k < kGramStride; ++k) {
                if (k < ng) {
                    const double t = wave_allsum_f64(g[k]);
                    if (tid == 0) a.gram[int64_t(blockIdx.x) * kGramStride + k] = t;
                }
            }
        }
        return;
    }
    // quads of the factor, then quads of the flat region; buffer bounds zero-fill a ragged tail
    const int64_t qf = (a.n + 3) / 4, qt = qf + (a.nflat + 3) / 4;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t q = int64_t(blockIdx.x) * kBlock + tid; q < qt; q += stride) {
        const bool fac = q < qf;
        const int64_t e0 = fac ? 4 * q : 4 * (q - qf);  // element index in dst / flat_dst
        const int64_t cnt = fac ? a.n : a.nflat;
        const int64_t base = fac ? 0 : a.flat_off;
        const uint32_t lim = uint32_t((base + cnt) * int64_t(sizeof(float)));
        float s[4];
        xchg_sum_quad(a, (base + e0) * int64_t(sizeof(float)), lim, s);
        float* d = fac ? a.dst : a.flat_dst;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < cnt) d[e0 + j] = s[j];
    }
}

hipError_t launch_xchg(const XchgArgs& a, hipStream_t s) {
    if (a.items) {
        k_xchg<<<a.nitems < 1 ? 1 : a.nitems, kBlock, 0, s>>>(a);
        return hipGetLastError();
    }
    const int64_t quads = (a.n + 3) / 4 + (a.nflat + 3) / 4;
    const int64_t blocks = (quads + kBlock - 1) / kBlock;
    // at least one workgroup (it raises the flag), at most one per CU
    k_xchg<<<int(blocks < 1 ? 1 : blocks < 256 ? blocks : 256), kBlock, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace psgd
