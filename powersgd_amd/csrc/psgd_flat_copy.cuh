// The flat tail's copy item of the fp32 destination-table final passes: psgd_apply_dst.hip
// (k_apply_dst, k_lowrank_dst) and psgd_wide_dst.hip (k_wide_apply_dst), whose leading workgroups run it.
#pragma once

#include "psgd_stream.cuh"

namespace psgd {

// Copy item: the item's elements of the all-reduced flat tail (`stage`, the flat plan's layout)
// to the tensor's own destination dst[en.tensor] (the flat plan's order; 4-byte aligned: element
// stores), bits unchanged. flat_round_item's shape without the rounding: the descriptor spans the
// item's elements of that tensor alone.
template <int NT>
__device__ __forceinline__ void flat_copy_item(const FlatArgs& a, const float* stage, int item, void* const* dst) {
    constexpr int PER = kFlatItem / NT;
    const FlatItem it = a.items[item];
    const FlatEntry en = a.entries[it.entry];
    const gptr<const float> x = gconst<float>(stage) + en.off;
    const uint32_t cnt = uint32_t(en.numel - it.start < kFlatItem ? en.numel - it.start : kFlatItem);
    const rsrc_t rf = make_rsrc(static_cast<float*>(dst[en.tensor]) + it.start, cnt * 4u);
    float v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t j = it.start + int64_t(q) * NT + threadIdx.x;
        v[q] = x[j < en.numel ? j : 0];  // clamped, unconditional
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) keep(v[q]);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t j = it.start + int64_t(q) * NT + threadIdx.x;
        if (j < en.numel) StIo<float>::st1(rf, uint32_t(int64_t(q) * NT + threadIdx.x) * 4u, v[q]);
    }
}

}  // namespace psgd
