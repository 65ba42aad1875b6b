// Two-shot all-reduce of one factor over IPC-mapped exchange buffers (k_xchg_rs, k_xchg_ag): the
// reduce-scatter + all-gather form of k_xchg (psgd_xchg.hip) for the large factors of wide plans
// (sessions of psgd_ipc_create2). Same slots, flags, nonces, bounded wait and arguments (XchgArgs).
//
// k_xchg makes every rank read all W slots whole: per exchange of n floats W * n floats, of which
// (W - 1) * n remote. Here rank r sums only its shard (n / W floats) of the W slots and the peers
// copy the finished shard: 2 * (W - 1) / W * n remote floats per rank, a factor W / 2 fewer.
//
// Protocol, per exchange of (step, iteration), on the iteration's flag word:
//  1. the producer kernels wrote the LOCAL factor into this rank's slot, write-through (st_slot;
//     psgd_xchg.cuh steps 1-2: the kernel boundary is the drain);
//  2. k_xchg_rs raises epoch 2 * (step + 1) - 1, waits for every peer's, and sums shard r of the W
//     slots in rank order (system-scope loads). The sum goes to `dst` and, IN PLACE, into shard r
//     of this rank's own slot, with the same write-through stores as (1). In place is safe: in
//     this phase only rank r reads shard r of any slot (rank q reads shard q), and a thread loads
//     a quad of its own slot before it stores that quad, so no load of this phase can see a sum;
//  3. k_xchg_ag is the next launch of the stream: the kernel boundary drains the stores of (2)
//     exactly as it drains those of (1). It raises epoch 2 * (step + 1), waits for every peer's,
//     and copies shard q of rank q's slot (system-scope loads) into `dst`, for every q != r. A
//     peer's flag at that epoch says its k_xchg_rs has completed, so the shard holds the sum. On
//     the last iteration it also sums the flat tail of the W slots one-shot, as k_xchg does (the
//     flat region is never written in place).
// Every rank therefore holds, element for element, the sum that rank `owner` formed in rank order:
// bitwise the one-shot result, on every rank.
//
// Slot reuse across steps is safe by the one-shot argument: the slot of (parity, iteration) is
// written again by the producers of step s + 2, which run after this rank passed every exchange of
// step s + 1; passing any exchange of step s + 1 requires every peer's flag of step s + 1, which a
// peer raises only after all its kernels of step s have completed (stream order), its k_xchg_ag
// copies of the in-place shards included. Within a step, the in-place shard of iteration `it` is
// read by peers in phase (3) only, and this rank does not write that slot again before step s + 2.
//
// A dead exchange (a wait gave up, now or earlier: xchg_arrive_and_wait) writes NaN: k_xchg_rs to
// its shard in `dst` AND in the slot, so a peer gathers NaN and never a plausible un-summed shard;
// k_xchg_ag to all of `dst` and `flat_dst`.
#include <hip/hip_runtime.h>

#include "psgd_xchg.cuh"

namespace psgd {

namespace {

typedef unsigned v4u_t __attribute__((ext_vector_type(4)));

// four consecutive floats of `dst` at element e0 (16-byte store where `al16` and the quad is whole)
__device__ __forceinline__ void xchg2_store_dst(float* dst, bool al16, int64_t e0, int64_t n, const float (&s)[4]) {
    if (al16 && e0 + 4 <= n) {
        *reinterpret_cast<float4*>(dst + e0) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) dst[e0 + j] = s[j];
    }
}

}  // namespace

__global__ __launch_bounds__(kBlock) void k_xchg_rs(XchgArgs a) {
    const bool dead = xchg_arrive_and_wait(a);
    const int64_t qf = (a.n + 3) / 4, per = xchg_shard_quads(a.n, a.world);
    const int64_t q0 = per * a.rank < qf ? per * a.rank : qf;
    const int64_t q1 = q0 + per < qf ? q0 + per : qf;
    const uint32_t lim = uint32_t(a.n * int64_t(sizeof(float)));  // < 2^32 (psgd_ipc_create2)
    float* slot = reinterpret_cast<float*>(const_cast<char*>(a.peers[a.rank]) + a.slot_off);
    const rsrc_t own = make_rsrc(slot, lim);
    const bool al16 = (reinterpret_cast<uintptr_t>(a.dst) & 15) == 0;
    const float nan = __builtin_nanf("");
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t q = q0 + int64_t(blockIdx.x) * kBlock + threadIdx.x; q < q1; q += stride) {
        const int64_t e0 = 4 * q;
        float s[4] = {nan, nan, nan, nan};
        // (the loads of this rank's own quad are among these: they return before the stores below)
        if (!dead) xchg_sum_quad(a, e0 * int64_t(sizeof(float)), lim, s);
        if (e0 + 4 <= a.n) {
            StIo<float>::template st4<kStAuxSlot>(own, uint32_t(e0 * int64_t(sizeof(float))), s);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < a.n) st_slot(slot + e0 + j, s[j]);
        }
        xchg2_store_dst(a.dst, al16, e0, a.n, s);
    }
}

__global__ __launch_bounds__(kBlock) void k_xchg_ag(XchgArgs a) {
    const int tid = threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int64_t g0 = int64_t(blockIdx.x) * kBlock + tid;
    if (xchg_arrive_and_wait(a)) {
        const float nan = __builtin_nanf("");
        for (int64_t i = g0; i < a.n + a.nflat; i += stride) {
            if (i < a.n) a.dst[i] = nan;
            else a.flat_dst[i - a.n] = nan;
        }
        return;
    }
    const int64_t qf = (a.n + 3) / 4, per = xchg_shard_quads(a.n, a.world);
    const uint32_t lim = uint32_t(a.n * int64_t(sizeof(float)));
    const bool al16 = (reinterpret_cast<uintptr_t>(a.dst) & 15) == 0;
    // quad i of every other rank's shard, kXchgUnroll owners' loads in flight together; an owner
    // past the last rank, or this rank itself, gets an empty descriptor (no access)
    for (int64_t i = g0; i < per; i += stride) {
        for (int w0 = 0; w0 < a.world; w0 += kXchgUnroll) {
            v4u_t v[kXchgUnroll];
#pragma unroll
            for (int u = 0; u < kXchgUnroll; ++u) {
                const int w = w0 + u;
                const bool on = w < a.world && w != a.rank;
                const rsrc_t rs = make_rsrc(a.peers[on ? w : a.rank] + a.slot_off, on ? lim : 0u);
                int64_t q = int64_t(w) * per + i;  // (a shard past the factor's end: clamped, not stored)
                q = q < qf ? q : qf - 1;
                v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, uint32_t(q * 16), 0, kSysAux);
            }
#pragma unroll
            for (int u = 0; u < kXchgUnroll; ++u) {
                const int w = w0 + u;
                const int64_t q = int64_t(w) * per + i;
                if (w < a.world && w != a.rank && q < qf) {
                    const float s[4] = {__uint_as_float(v[u][0]), __uint_as_float(v[u][1]), __uint_as_float(v[u][2]),
                                        __uint_as_float(v[u][3])};
                    xchg2_store_dst(a.dst, al16, 4 * q, a.n, s);
                }
            }
        }
    }
    // the flat tail (last iteration): summed one-shot, exactly as k_xchg's flat quads
    const int64_t qfl = (a.nflat + 3) / 4;
    const uint32_t flim = uint32_t((a.flat_off + a.nflat) * int64_t(sizeof(float)));
    for (int64_t q = g0; q < qfl; q += stride) {
        const int64_t e0 = 4 * q;
        float s[4];
        xchg_sum_quad(a, (a.flat_off + e0) * int64_t(sizeof(float)), flim, s);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < a.nflat) a.flat_dst[e0 + j] = s[j];
    }
}

namespace {
// at least one workgroup (it raises the flag), at most one per CU, as launch_xchg
int xchg2_blocks(int64_t quads) {
    const int64_t blocks = (quads + kBlock - 1) / kBlock;
    return int(blocks < 1 ? 1 : blocks < 256 ? blocks : 256);
}
}  // namespace

hipError_t launch_xchg_rs(const XchgArgs& a, hipStream_t s) {
    XchgArgs r = a;
    r.flat_dst = nullptr;
    r.nflat = 0;
    k_xchg_rs<<<xchg2_blocks(xchg_shard_quads(a.n, a.world)), kBlock, 0, s>>>(r);
    return hipGetLastError();
}

hipError_t launch_xchg_ag(const XchgArgs& a, hipStream_t s) {
    const int64_t per = xchg_shard_quads(a.n, a.world), qfl = (a.nflat + 3) / 4;
    k_xchg_ag<<<xchg2_blocks(per > qfl ? per : qfl), kBlock, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace psgd
