// The flat tail's update items of the fused SGD steps: the leading workgroups of the final launch
// (k_apply_sgd / k_lowrank_sgd, psgd_sgd_dst.hip; k_wide_apply_sgd, psgd_wide_sgd.hip; their
// master-weight forms) apply THE UPDATE to the flat plan's tensors from the all-reduced fp32 stage.
#pragma once

#include "psgd_stream.cuh"

namespace psgd {

// Update item of the flat tail: g is the item's elements of the all-reduced stage (the flat plan's
// layout), p / buf the tensor's own (4-byte aligned: element accesses). flat_copy_item's shape: the
// descriptors span the item's elements of that tensor alone, every load is issued before the
// first store.
template <int NT>
__device__ __forceinline__ void flat_sgd_item(const FlatArgs& a, const SgdDst& x, int item) {
    constexpr int PER = kFlatItem / NT;
    const FlatItem it = a.items[item];
    const FlatEntry en = a.entries[it.entry];
    const psgd_sgd_hyper h = x.hyper[x.unc0 + en.tensor];
    const bool mom = h.momentum != 0.f;
    const gptr<const float> st = gconst<float>(x.stage) + en.off;
    const uint32_t cnt = uint32_t(en.numel - it.start < kFlatItem ? en.numel - it.start : kFlatItem);
    const rsrc_t rP = make_rsrc(static_cast<float*>(x.unc_p[en.tensor]) + it.start, cnt * 4u);
    const rsrc_t rB = make_rsrc(mom ? static_cast<float*>(x.unc_buf[en.tensor]) + it.start : nullptr, mom ? cnt * 4u : 0u);
    float g[PER], p[PER], b[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t j = it.start + int64_t(q) * NT + threadIdx.x;
        const uint32_t off = uint32_t(int64_t(q) * NT + threadIdx.x) * 4u;
        g[q] = st[j < en.numel ? j : 0];  // clamped, unconditional
        p[q] = BufIo<float>::ld1(rP, off);  // past the item: zeros, no access
        b[q] = BufIo<float>::ld1(rB, off);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        keep(g[q]);
        keep(p[q]);
        keep(b[q]);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t off = uint32_t(int64_t(q) * NT + threadIdx.x) * 4u;
        sgd_update(h, g[q], p[q], b[q]);
        StIo<float>::st1<0>(rP, off, p[q]);  // past the item: dropped by the descriptor
        if (mom) StIo<float>::st1<0>(rB, off, b[q]);
    }
}

// flat_sgd_item plus the bf16 store (the master-weight steps: k_apply_sgd_mp / k_lowrank_sgd_mp,
// psgd_sgd_mp_dst.hip; k_wide_apply_sgd_mp, psgd_wide_sgd.hip): p / buf the flat plan's tensor's own
// master and buffer (4-byte accesses), w its bf16 model tensor (2-byte stores, a descriptor over the
// item's elements in 2-byte units; offsets past the item are kOob by an explicit test).
template <int NT>
__device__ __forceinline__ void flat_sgd_mp_item(const FlatArgs& a, const SgdMpDst& y, int item) {
    constexpr int PER = kFlatItem / NT;
    const SgdDst& x = y.x;
    const FlatItem it = a.items[item];
    const FlatEntry en = a.entries[it.entry];
    const psgd_sgd_hyper h = x.hyper[x.unc0 + en.tensor];
    const bool mom = h.momentum != 0.f;
    const gptr<const float> st = gconst<float>(x.stage) + en.off;
    const uint32_t cnt = uint32_t(en.numel - it.start < kFlatItem ? en.numel - it.start : kFlatItem);
    const rsrc_t rP = make_rsrc(static_cast<float*>(x.unc_p[en.tensor]) + it.start, cnt * 4u);
    const rsrc_t rB = make_rsrc(mom ? static_cast<float*>(x.unc_buf[en.tensor]) + it.start : nullptr, mom ? cnt * 4u : 0u);
    const rsrc_t rW = make_rsrc(static_cast<uint16_t*>(y.unc_w[en.tensor]) + it.start, cnt * 2u);
    float g[PER], p[PER], b[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t j = it.start + int64_t(q) * NT + threadIdx.x;
        const uint32_t off = uint32_t(int64_t(q) * NT + threadIdx.x) * 4u;
        g[q] = st[j < en.numel ? j : 0];  // clamped, unconditional
        p[q] = BufIo<float>::ld1(rP, off);  // past the item: zeros, no access
        b[q] = BufIo<float>::ld1(rB, off);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        keep(g[q]);
        keep(p[q]);
        keep(b[q]);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t e = uint32_t(int64_t(q) * NT + threadIdx.x);
        sgd_update(h, g[q], p[q], b[q]);
        StIo<float>::st1<0>(rP, e * 4u, p[q]);  // past the item: dropped by the descriptor
        if (mom) StIo<float>::st1<0>(rB, e * 4u, b[q]);
        StIo<bf16_pin_t>::st1<0>(rW, e < cnt ? e * 2u : kOob, p[q]);
    }
}

}  // namespace psgd
