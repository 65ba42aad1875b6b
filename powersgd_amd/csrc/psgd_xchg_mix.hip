// The mixed tail of the one-shot all-reduce over IPC-mapped exchange buffers (k_xchg_mix): the
// LAST exchange of psgd_aggregate_mixed_ipc[_dst] on a step with uncompressed tensors. The flag
// and wait protocol is k_xchg's (psgd_xchg.cuh), and so is the factor part; the flat region of the
// W slots is summed per flat item of the flat plan and stored as bf16 where the averages belong,
// so the fp32 flat sums never reach memory and nothing rounds them in a later pass.
#include <hip/hip_runtime.h>

#include "psgd_xchg.cuh"

namespace psgd {

// One flat item (at most kFlatItem consecutive elements of one uncompressed tensor): element j of
// the item is the rank-order sum s = x0; s += x1; ... of the W peers' slot values (xchg_sum_quad's
// order, so the sums are k_xchg's bit for bit), stored as f2bf(s): the run-table GATHER of the
// three-stage flow. DST: at the tensor's own destination (2-byte aligned: element stores), else in
// the dense bf16 flat buffer at the flat plan's offset. Both descriptors span the item's elements
// alone: a load or store past them is dropped. `dead`: bf16 NaN to every element of the item.
template <bool DST>
__device__ __forceinline__ void xchg_flat_item(const XchgArgs& a, const XchgMixArgs& m, int item, bool dead) {
    constexpr int PER = kFlatItem / kBlock;
    const FlatItem it = m.items[item];
    const FlatEntry en = m.entries[it.entry];
    const uint32_t cnt = uint32_t(en.numel - it.start < kFlatItem ? en.numel - it.start : kFlatItem);
    bf16_t* fbase;
    if constexpr (DST) fbase = static_cast<bf16_t*>(m.unc_dst[en.tensor]) + it.start;
    else fbase = static_cast<bf16_t*>(m.flat_out) + en.off + it.start;
    const rsrc_t rf = make_rsrc(fbase, cnt * 2u);
    float s[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) s[q] = __builtin_nanf("");
    if (!dead) {
        // byte offset of the item's first element in every rank's exchange buffer
        const int64_t src = a.slot_off + (a.flat_off + en.off + it.start) * int64_t(sizeof(float));
        for (int w0 = 0; w0 < a.world; w0 += kXchgUnroll) {
            float v[kXchgUnroll][PER];
#pragma unroll
            for (int u = 0; u < kXchgUnroll; ++u) {
                // uniform guard: no load past the last peer (and a clamped table index behind an
                // empty descriptor, should the loads ever be hoisted over it)
                const bool on = w0 + u < a.world;
                const rsrc_t rs = make_rsrc(a.peers[on ? w0 + u : w0] + src, on ? cnt * 4u : 0u);
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    v[u][q] = 0.f;
                    if (on)
                        v[u][q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                            rs, uint32_t(q * kBlock + int(threadIdx.x)) * 4u, 0, kSysAux));
                }
            }
#pragma unroll
            for (int u = 0; u < kXchgUnroll; ++u)
                if (w0 + u < a.world)
#pragma unroll
                    for (int q = 0; q < PER; ++q) s[q] = w0 + u == 0 ? v[u][q] : s[q] + v[u][q];  // rank order
        }
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t e = uint32_t(q * kBlock + int(threadIdx.x));
        if (e < cnt) StIo<bf16_t>::st1(rf, e * 2u, s[q]);
    }
}

template <bool DST>
__global__ __launch_bounds__(kBlock) void k_xchg_mix(XchgArgs a, XchgMixArgs m) {
    const int tid = threadIdx.x;
    const bool dead = xchg_arrive_and_wait(a);
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    if (dead) {
        // an invalid exchange returns NaN sums, never plausible stale ones: fp32 NaN to the factor,
        // bf16 NaN (below) to the flat destinations of this workgroup's share
        const float nan = __builtin_nanf("");
        for (int64_t i = int64_t(blockIdx.x) * kBlock + tid; i < a.n; i += stride) a.dst[i] = nan;
    } else {
        // quads of the factor; buffer bounds zero-fill a ragged tail
        const int64_t qf = (a.n + 3) / 4;
        const uint32_t lim = uint32_t(a.n * int64_t(sizeof(float)));
        for (int64_t q = int64_t(blockIdx.x) * kBlock + tid; q < qf; q += stride) {
            float s[4];
            xchg_sum_quad(a, 4 * q * int64_t(sizeof(float)), lim, s);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < a.n) a.dst[4 * q + j] = s[j];
        }
    }
    for (int item = blockIdx.x; item < m.nitems; item += int(gridDim.x)) xchg_flat_item<DST>(a, m, item, dead);
}

hipError_t launch_xchg_mix(const XchgArgs& a, const XchgMixArgs& m, bool dst, hipStream_t s) {
    const int64_t blocks = ((a.n + 3) / 4 + kBlock - 1) / kBlock + m.nitems;
    // at least one workgroup (it raises the flag), at most one per CU
    const int grid = int(blocks < 1 ? 1 : blocks < 256 ? blocks : 256);
    if (dst) k_xchg_mix<true><<<grid, kBlock, 0, s>>>(a, m);
    else k_xchg_mix<false><<<grid, kBlock, 0, s>>>(a, m);
    return hipGetLastError();
}

}  // namespace psgd
