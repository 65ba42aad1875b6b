// Kernel instances of psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst (DirectDst, psgd_internal.h):
// the final passes of the communicator and IPC sequences of an fp32 plan, rank buckets 1-32, with
// the fp32 averages stored at per-tensor destinations (views into DDP buckets, 4-byte aligned or
// better) instead of the output slab. Each is its dense instance (k_apply<float, R, NI, SHARED,
// ONT>, k_lowrank_out<float, R, NI>) with DST set: the same tiles, loads and fp32 arithmetic. The
// layout follows the gradients and the plan's offsets, never the destination; the store of a
// vector tile (the VALU tiles' 4-column vectors, the matrix-core tiles' row quads) is 16 bytes
// when the tile's first destination element is 16-byte aligned, else four 4-byte stores: two
// copies of the tile body, chosen once per tile, workgroup-uniform. Every store goes through a
// descriptor that spans the tile's rows of its own tensor: nothing can land on a bucket neighbour.
#include "psgd_final.cuh"

namespace psgd {

// true when the tile's first destination element (tensor base + row offset; with m % 4 == 0 every
// vector of the tile then) is 16-byte aligned. Workgroup-uniform: one test per tile.
__device__ __forceinline__ bool dst_al16(const ApplyArgs& a, const MatDesc& d, const Tile& t) {
    const uintptr_t o = reinterpret_cast<uintptr_t>(a.odst[d.tensor]) +
                        uintptr_t(int64_t(t.chunk) * d.chunk_rows * d.m) * sizeof(float);
    return (o & 15) == 0;
}

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

// k_apply<float, R, NI, SHARED, ONT> into a.odst; the copy items of the flat tail are its leading
// workgroups
template <int R, int NI, bool SHARED, bool ONT>
__global__ __launch_bounds__(kBlock) void k_apply_dst(ApplyArgs a, const float* stage, void* const* unc_dst) {
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_copy_item<kBlock>(a.flat, stage, blockIdx.x, unc_dst);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    if constexpr (R <= 8) {
        if (d.vec) {
            if (dst_al16(a, d, t))
                apply_tile<float, R, NI, SHARED, 4, ONT, float, kDstVec>(a, d, t);
            else
                apply_tile<float, R, NI, SHARED, 4, ONT, float, kDstElem>(a, d, t);
            return;
        }
    }
    if constexpr (R >= 16) {
        __shared__ __attribute__((aligned(16))) float qs[ApplyMfmaLds<R>::floats];
        constexpr int NS = SHARED ? 1 : 2;
        // k_apply's choice between the matrix-core tile and its VALU fallback, with the slab's
        // term (a 16-byte aligned buffer + the plan's offset) in the destination's place: the
        // arithmetic is the dense instance's wherever the bucket view lies
        const uintptr_t rows = reinterpret_cast<uintptr_t>(a.grads[t.tensor]) |
                               reinterpret_cast<uintptr_t>(a.rdst ? a.rdst[d.tensor] : a.grads[t.tensor]) |
                               uintptr_t(d.out_off) * sizeof(float);
        if ((d.m & 3) == 0 && (rows & (4 * sizeof(float) - 1)) == 0 && a.nterms * NS <= kApplyMfmaSets) {
            if (dst_al16(a, d, t))
                apply_tile_mfma<float, R, SHARED, ONT, kDstVec>(a, d, t, qs);
            else
                apply_tile_mfma<float, R, SHARED, ONT, kDstElem>(a, d, t, qs);
            return;
        }
    }
    apply_tile<float, R, NI, SHARED, 1, ONT, float, kDstVec>(a, d, t);
}

// k_lowrank_out<float, R, NI> (the output pass after a fused k_final_odd) likewise
template <int R, int NI>
__global__ __launch_bounds__(kBlock) void k_lowrank_dst(ApplyArgs a, const float* stage, void* const* unc_dst) {
    static_assert(R <= 2, "k_final_odd's K-term form: rank buckets 1 and 2");
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_copy_item<kBlock>(a.flat, stage, blockIdx.x, unc_dst);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    if (!d.vec)
        lowrank_tile<float, R, NI, 1, kDstVec>(a, d, t);
    else if (dst_al16(a, d, t))
        lowrank_tile<float, R, NI, 4, kDstVec>(a, d, t);
    else
        lowrank_tile<float, R, NI, 4, kDstElem>(a, d, t);
}

namespace {

template <typename F>
hipError_t ask_or_launch(F fn, int nblocks, hipStream_t s, int* waves, const ApplyArgs& a, const DirectDst& t) {
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    if (nblocks == 0) return hipSuccess;
    timed_launch(fn, dim3(nblocks), dim3(kBlock), s, a, static_cast<const float*>(t.stage), t.unc_dst);
    return hipGetLastError();
}

// the instance dispatch_apply_r<float, R> picks: the same NI, SHARED and ONT
template <int R>
hipError_t dispatch_apply_dst(int nterms, bool shared, const ApplyArgs& a, const DirectDst& t, int ntiles,
                              hipStream_t s, int* waves) {
    const int nb = ntiles + a.flat.nitems;
    auto go = [&](auto N) -> hipError_t {
        constexpr int NN = decltype(N)::value;
        if (shared && a.out_nt) return ask_or_launch(&k_apply_dst<R, NN, true, true>, nb, s, waves, a, t);
        if (shared) return ask_or_launch(&k_apply_dst<R, NN, true, false>, nb, s, waves, a, t);
        return ask_or_launch(&k_apply_dst<R, NN, false, false>, nb, s, waves, a, t);
    };
    if constexpr (R <= 8) return by_ni<1, 2, 3, 4>(apply_ni(R, nterms, shared), go);
    else return by_ni<>(-1, go);
}

// the instance dispatch_lowrank_r<float, R> picks
template <int R>
hipError_t dispatch_lowrank_dst(int nterms, const ApplyArgs& a, const DirectDst& t, int ntiles, hipStream_t s,
                                int* waves) {
    return by_ni<1, 2, 4>(lowrank_ni(R, nterms), [&](auto N) -> hipError_t {
        return ask_or_launch(&k_lowrank_dst<R, decltype(N)::value>, ntiles + a.flat.nitems, s, waves, a, t);
    });
}

}  // namespace

hipError_t launch_apply_dst(int R, int nterms, bool shared, const ApplyArgs& a, const DirectDst& t, int ntiles,
                            hipStream_t s, int* waves) {
    switch (R) {
        case 1: return dispatch_apply_dst<1>(nterms, shared, a, t, ntiles, s, waves);
        case 2: return dispatch_apply_dst<2>(nterms, shared, a, t, ntiles, s, waves);
        case 4: return dispatch_apply_dst<4>(nterms, shared, a, t, ntiles, s, waves);
        case 8: return dispatch_apply_dst<8>(nterms, shared, a, t, ntiles, s, waves);
        case 16: return dispatch_apply_dst<16>(nterms, shared, a, t, ntiles, s, waves);
        case 32: return dispatch_apply_dst<32>(nterms, shared, a, t, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_lowrank_dst(int R, int nterms, const ApplyArgs& a, const DirectDst& t, int ntiles, hipStream_t s,
                              int* waves) {
    switch (R) {
        case 1: return dispatch_lowrank_dst<1>(nterms, a, t, ntiles, s, waves);
        case 2: return dispatch_lowrank_dst<2>(nterms, a, t, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace psgd
