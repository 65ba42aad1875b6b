// The flag and wait protocol of the one-shot all-reduce over IPC-mapped exchange buffers, shared by
// its kernels (k_xchg, psgd_xchg.hip; k_xchg_mix, psgd_xchg_mix.hip) and by the two-shot form's
// (k_xchg_rs, k_xchg_ag, psgd_xchg2.hip), and the rank-order sum of a 16-byte quad of the W slots.
#pragma once

#include <hip/hip_runtime.h>

#include "psgd_internal.h"
#include "psgd_stream.cuh"

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

// Raise this rank's epoch flag (workgroup 0), wait (bounded) for every peer's. True, for the whole
// workgroup: the exchange is dead (a wait gave up, now or in an earlier exchange of this rank) and
// the caller writes NaN sums, never plausible stale ones.
__device__ __forceinline__ bool xchg_arrive_and_wait(const XchgArgs& a) {
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
    return __syncthreads_or(dead);
}

}  // namespace psgd
