// One-shot all-reduce over IPC-mapped exchange buffers (k_xchg).
#include <hip/hip_runtime.h>

#include "psgd_internal.h"
#include "psgd_stream.cuh"
#include "psgd_chain.cuh"  // wave_allsum_f64

namespace psgd {

// The reference's SUM all-reduce of an out-factor (powersgd.py:204-209), one node, one
// process per GPU, stream-ordered with no host round trip. Cross-GPU visibility, step by step:
//  1. the kernels before this one wrote the LOCAL factor into this rank's exchange slot with
//     system-scope stores (st_slot: `sc0 sc1`, write-through; the flat region with PSGD_ST_AUX
//     = sc0 | nt | sc1): no byte of the slot waits in any of the eight L2s for a writeback;
//  2. this launch starts only after they completed (same stream, barrier bit): every one of those
//     stores has been acknowledged by memory;
//  3. workgroup 0 then stores this rank's epoch flag (system scope, `sc0 sc1`);
//  4. peers poll the flag with system-scope loads and read the slot ONLY with system-scope loads
//     (`sc0 sc1`, which no non-coherent cache level serves), so they see the bytes of (1).
// This is the write-through hand-off of MI355X_MICROARCH.md (visibility table, first row: stores
// all write-through, drained before ONE lane's flag store, flag polled and payload loaded with
// coherent loads) at system scope, with the kernel boundary as the drain. It needs no release
// fence: one here would write back only this workgroup's XCD L2, which (1) leaves clean.
// The wait is bounded: a peer that never arrives sets the sticky error word (host-mapped, read by
// the next psgd_aggregate_ipc call, which then fails) instead of hanging the queue.
#ifndef PSGD_XCHG_FLAG_ORDER
#define PSGD_XCHG_FLAG_ORDER __ATOMIC_RELAXED
#endif
// System-scope (sc0 | sc1) 16-byte loads: they miss in every non-coherent cache level.
constexpr int kSysAux = 17;
constexpr int kXchgUnroll = 8;  // peers whose loads are in flight together

__device__ __forceinline__ void xchg_sum_quad(const XchgArgs& a, int64_t src_byte, uint32_t lim, float (&s)[4]) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    for (int w0 = 0; w0 < a.world; w0 += kXchgUnroll) {
        v4u v[kXchgUnroll];
#pragma unroll
        for (int u = 0; u < kXchgUnroll; ++u) {
            const bool on = w0 + u < a.world;  // past the last peer: an empty descriptor, no access
            const rsrc_t rs = make_rsrc(a.peers[on ? w0 + u : w0] + a.slot_off, on ? lim : 0u);
            v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, uint32_t(src_byte), 0, kSysAux);
        }
#pragma unroll
        for (int u = 0; u < kXchgUnroll; ++u)
            if (w0 + u < a.world)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = __uint_as_float(v[u][j]);
                    s[j] = w0 + u == 0 ? x : s[j] + x;  // rank order
                }
    }
}

__global__ __launch_bounds__(kBlock) void k_xchg(XchgArgs a) {
    const int tid = threadIdx.x;
    // the slot bytes were written through by the PREVIOUS kernels of this stream (steps 1-2
    // above): the flag is a plain system-scope store, no fence
    if (blockIdx.x == 0 && tid == 0)
        __hip_atomic_store(a.own_flag, (uint64_t(a.own_nonce) << 32) | a.epoch, PSGD_XCHG_FLAG_ORDER,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    bool dead = false;
    if (tid < a.world && tid != a.rank) {  // lane w polls peer w: the W round trips overlap
        const uint64_t* f = reinterpret_cast<const uint64_t*>(a.peers[tid] + a.flag_off);
        const uint32_t want = a.nonces[tid];  // this session's flags only
        uint32_t spins = 0;
        for (;;) {
            // the device copy of the sticky error word, loaded beside the flag (no extra round
            // trip): an earlier exchange of this rank gave up, so the ranks' epochs have drifted
            // apart and this exchange is invalid whatever the flags say
            const int32_t gone = __hip_atomic_load(a.err_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t fv = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (gone) {
                dead = true;
                break;
            }
            if (uint32_t(fv >> 32) == want && (fv & 0xffffffffull) >= a.epoch) break;
            if (++spins > a.spin_limit) {
                // host-mapped sticky word (vector store, system scope) and its device copy: the
                // results of this step are invalid and the host refuses every later exchange step
                __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(a.err_dev, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                dead = true;
                break;
            }
            __builtin_amdgcn_s_sleep(10);
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    if (__syncthreads_or(dead)) {
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
