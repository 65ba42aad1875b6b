// The flat tail's update items of the fused Adam steps: the leading workgroups of the final launch
// (k_apply_adam / k_lowrank_adam, psgd_adam_dst.hip; their master-weight forms, psgd_adam_mp_dst.hip;
// k_wide_apply_adam, psgd_wide_adam.hip) apply THE UPDATE to the flat plan's tensors from the
// all-reduced fp32 stage.
#pragma once

#include "psgd_stream.cuh"

namespace psgd {

// Update item of the flat tail: g is the item's elements of the all-reduced stage (the flat plan's
// layout), p / m / v the tensor's own (4-byte aligned: element accesses). flat_sgd_item's shape: the
// descriptors span the item's elements of that tensor alone, every load is issued before the
// first store.
template <int NT>
__device__ __forceinline__ void flat_adam_item(const FlatArgs& a, const AdamDst& x, int item) {
    constexpr int PER = kFlatItem / NT;
    const FlatItem it = a.items[item];
    const FlatEntry en = a.entries[it.entry];
    const psgd_adam_hyper h = x.hyper[x.unc0 + en.tensor];
    const gptr<const float> st = gconst<float>(x.stage) + en.off;
    const uint32_t cnt = uint32_t(en.numel - it.start < kFlatItem ? en.numel - it.start : kFlatItem);
    const rsrc_t rP = make_rsrc(static_cast<float*>(x.unc_p[en.tensor]) + it.start, cnt * 4u);
    const rsrc_t rM = make_rsrc(static_cast<float*>(x.unc_m[en.tensor]) + it.start, cnt * 4u);
    const rsrc_t rV = make_rsrc(static_cast<float*>(x.unc_v[en.tensor]) + it.start, cnt * 4u);
    float g[PER], p[PER], m[PER], v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t j = it.start + int64_t(q) * NT + threadIdx.x;
        const uint32_t off = uint32_t(int64_t(q) * NT + threadIdx.x) * 4u;
        g[q] = st[j < en.numel ? j : 0];  // clamped, unconditional
        p[q] = BufIo<float>::ld1(rP, off);  // past the item: zeros, no access
        m[q] = BufIo<float>::ld1(rM, off);
        v[q] = BufIo<float>::ld1(rV, off);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        keep(g[q]);
        keep(p[q]);
        keep(m[q]);
        keep(v[q]);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t off = uint32_t(int64_t(q) * NT + threadIdx.x) * 4u;
        adam_update(h, g[q], p[q], m[q], v[q]);
        StIo<float>::st1<0>(rP, off, p[q]);  // past the item: dropped by the descriptor
        StIo<float>::st1<0>(rM, off, m[q]);
        StIo<float>::st1<0>(rV, off, v[q]);
    }
}

// flat_adam_item plus the bf16 store: g is the item's elements of the all-reduced stage, p / m / v the
// flat plan's tensor's own masters and moments (4-byte accesses), w its bf16 model tensor (2-byte
// stores). The descriptors span the item's elements of that tensor alone and every load is issued
// before the first store.
template <int NT>
__device__ __forceinline__ void flat_adam_mp_item(const FlatArgs& a, const AdamMpDst& y, int item) {
    constexpr int PER = kFlatItem / NT;
    const AdamDst& x = y.x;
    const FlatItem it = a.items[item];
    const FlatEntry en = a.entries[it.entry];
    const psgd_adam_hyper h = x.hyper[x.unc0 + en.tensor];
    const gptr<const float> st = gconst<float>(x.stage) + en.off;
    const uint32_t cnt = uint32_t(en.numel - it.start < kFlatItem ? en.numel - it.start : kFlatItem);
    const rsrc_t rP = make_rsrc(static_cast<float*>(x.unc_p[en.tensor]) + it.start, cnt * 4u);
    const rsrc_t rM = make_rsrc(static_cast<float*>(x.unc_m[en.tensor]) + it.start, cnt * 4u);
    const rsrc_t rV = make_rsrc(static_cast<float*>(x.unc_v[en.tensor]) + it.start, cnt * 4u);
    const rsrc_t rW = make_rsrc(static_cast<uint16_t*>(y.unc_w[en.tensor]) + it.start, cnt * 2u);
    float g[PER], p[PER], m[PER], v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t j = it.start + int64_t(q) * NT + threadIdx.x;
        const uint32_t off = uint32_t(int64_t(q) * NT + threadIdx.x) * 4u;
        g[q] = st[j < en.numel ? j : 0];  // clamped, unconditional
        p[q] = BufIo<float>::ld1(rP, off);  // past the item: zeros, no access
        m[q] = BufIo<float>::ld1(rM, off);
        v[q] = BufIo<float>::ld1(rV, off);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        keep(g[q]);
        keep(p[q]);
        keep(m[q]);
        keep(v[q]);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t e = uint32_t(int64_t(q) * NT + threadIdx.x);
        adam_update(h, g[q], p[q], m[q], v[q]);
        StIo<float>::st1<0>(rP, e * 4u, p[q]);  // past the item: dropped by the descriptor
        StIo<float>::st1<0>(rM, e * 4u, m[q]);
        StIo<float>::st1<0>(rV, e * 4u, v[q]);
        StIo<bf16_pin_t>::st1<0>(rW, e < cnt ? e * 2u : kOob, p[q]);
    }
}

}  // namespace psgd
