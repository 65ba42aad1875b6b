// Kernel instances of psgd_aggregate_mixed_comm_dst (MixDst, psgd_internal.h): the three final
// passes of the communicator sequence on an fp32 residual, with the bf16 averages stored at
// per-tensor destinations (views into DDP buckets, 2-byte aligned or better) instead of a dense
// buffer. Each is its dense instance (k_apply_mix_w, k_lowrank_mix, k_apply_mix) with DST set:
// the same tiles, loads and fp32 arithmetic (the layout follows the residual, never the
// destination), the same bf16_pin_t pinning; the store of a vector tile is 8 bytes when the tile's
// destination is 8-byte aligned, else four 2-byte stores: two copies of the tile body, chosen once
// per tile (one body with both store forms behind a branch cost up to 50 VGPRs). Every store goes
// through a descriptor that spans the tile's rows of its own tensor: nothing can land on a
// bucket neighbour.
#include "psgd_final.cuh"

namespace psgd {

// k_apply_mix_w<R, NI> (W > 1, two term sets) into a.odst; the round items of the flat tail, into
// unc_dst, are its leading workgroups
template <int R, int NI>
__global__ __launch_bounds__(kBlock) void k_apply_mix_w_dst(ApplyArgs a, MixArgs x, void* const* unc_dst) {
    static_assert(R <= 4, "mixed instances: rank buckets 1, 2 and 4");
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_round_item<kBlock, true>(a.flat, x.stage, blockIdx.x, unc_dst);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    if (!d.vec)
        apply_tile<float, R, NI, false, 1, false, bf16_pin_t, kDstVec>(a, d, t);
    else if (dst_al8(a, d, t))
        apply_tile<float, R, NI, false, 4, false, bf16_pin_t, kDstVec>(a, d, t);
    else
        apply_tile<float, R, NI, false, 4, false, bf16_pin_t, kDstElem>(a, d, t);
}

// k_lowrank_mix<R, NI> (the output pass after a fused k_final_odd) likewise
template <int R, int NI>
__global__ __launch_bounds__(kBlock) void k_lowrank_mix_dst(ApplyArgs a, MixArgs x, void* const* unc_dst) {
    static_assert(R <= 2, "k_final_odd's K-term form: rank buckets 1 and 2");
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_round_item<kBlock, true>(a.flat, x.stage, blockIdx.x, unc_dst);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    if (!d.vec)
        lowrank_tile<bf16_pin_t, R, NI, 1, kDstVec>(a, d, t);
    else if (dst_al8(a, d, t))
        lowrank_tile<bf16_pin_t, R, NI, 4, kDstVec>(a, d, t);
    else
        lowrank_tile<bf16_pin_t, R, NI, 4, kDstElem>(a, d, t);
}

// k_apply_mix<R, NI, ONT> (shared terms: the unfused final pass of a 1-rank communicator) into
// a.odst. No flat items: k_apply_mix's ingest, and the round runs after it (k_flat_round_dst)
template <int R, int NI, bool ONT>
__global__ __launch_bounds__(kBlock) void k_apply_mix_dst(ApplyArgs a) {
    static_assert(R <= 4, "mixed instances: rank buckets 1, 2 and 4");
    const Tile t = a.tiles[blockIdx.x];
    const MatDesc d = a.mats[t.mat];
    if (!d.vec)
        apply_tile<float, R, NI, true, 1, ONT, bf16_pin_t, kDstVec>(a, d, t);
    else if (dst_al8(a, d, t))
        apply_tile<float, R, NI, true, 4, ONT, bf16_pin_t, kDstVec>(a, d, t);
    else
        apply_tile<float, R, NI, true, 4, ONT, bf16_pin_t, kDstElem>(a, d, t);
}

__global__ __launch_bounds__(kBlock) void k_flat_round_dst(FlatArgs a, MixArgs x, void* const* unc_dst) {
    flat_round_item<kBlock, true>(a, x.stage, blockIdx.x, unc_dst);
}

namespace {

// `waves` (if non-null) receives the resident waves per SIMD of the instance that would run; no
// tiles and no flat items: no launch
template <typename F, typename... Args>
hipError_t ask_or_launch(F fn, int nblocks, hipStream_t s, int* waves, Args... args) {
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    if (nblocks == 0) return hipSuccess;
    timed_launch(fn, dim3(nblocks), dim3(kBlock), s, args...);
    return hipGetLastError();
}

template <int R>
hipError_t dispatch_apply_mix_w_dst(int nterms, const ApplyArgs& a, const MixArgs& x, void* const* unc_dst, int ntiles,
                                    hipStream_t s, int* waves) {
    auto go = [&](auto N) -> hipError_t {
        return ask_or_launch(&k_apply_mix_w_dst<R, decltype(N)::value>, ntiles + a.flat.nitems, s, waves, a, x, unc_dst);
    };
    // the register-cached term counts of dispatch_apply_mix_w (psgd_stream.cuh): the same NI
    if constexpr (R <= 2) return by_ni<1, 2, 3, 4>(apply_ni(R, nterms, false), go);
    else return by_ni<1, 2, 3>(apply_ni(R, nterms, false), go);
}

template <int R>
hipError_t dispatch_lowrank_mix_dst(int nterms, const ApplyArgs& a, const MixArgs& x, void* const* unc_dst, int ntiles,
                                    hipStream_t s, int* waves) {
    return by_ni<1, 2, 4>(lowrank_ni(R, nterms), [&](auto N) -> hipError_t {
        return ask_or_launch(&k_lowrank_mix_dst<R, decltype(N)::value>, ntiles + a.flat.nitems, s, waves, a, x, unc_dst);
    });
}

template <int R>
hipError_t dispatch_apply_mix_dst(int nterms, const ApplyArgs& a, int ntiles, hipStream_t s, int* waves) {
    auto go = [&](auto N, auto ONT) -> hipError_t {
        return ask_or_launch(&k_apply_mix_dst<R, decltype(N)::value, decltype(ONT)::value>, ntiles, s, waves, a);
    };
    return by_ni<1, 2, 3, 4>(apply_ni(R, nterms, true), [&](auto N) {
        return a.out_nt ? go(N, std::true_type{}) : go(N, std::false_type{});
    });
}

}  // namespace

hipError_t launch_apply_mix_w_dst(int R, int nterms, const ApplyArgs& a, const MixArgs& x, void* const* unc_dst,
                                  int ntiles, hipStream_t s, int* waves) {
    switch (R) {
        case 1: return dispatch_apply_mix_w_dst<1>(nterms, a, x, unc_dst, ntiles, s, waves);
        case 2: return dispatch_apply_mix_w_dst<2>(nterms, a, x, unc_dst, ntiles, s, waves);
        case 4: return dispatch_apply_mix_w_dst<4>(nterms, a, x, unc_dst, ntiles, s, waves);
        case 16:
        case 32: return launch_apply_mix_w_dst_mc(R, a, x, unc_dst, ntiles, s, waves);  // psgd_mixed_mfma.hip
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_lowrank_mix_dst(int R, int nterms, const ApplyArgs& a, const MixArgs& x, void* const* unc_dst,
                                  int ntiles, hipStream_t s, int* waves) {
    switch (R) {
        case 1: return dispatch_lowrank_mix_dst<1>(nterms, a, x, unc_dst, ntiles, s, waves);
        case 2: return dispatch_lowrank_mix_dst<2>(nterms, a, x, unc_dst, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_apply_mix_dst(int R, int nterms, const ApplyArgs& a, int ntiles, hipStream_t s, int* waves) {
    switch (R) {
        case 1: return dispatch_apply_mix_dst<1>(nterms, a, ntiles, s, waves);
        case 2: return dispatch_apply_mix_dst<2>(nterms, a, ntiles, s, waves);
        case 4: return dispatch_apply_mix_dst<4>(nterms, a, ntiles, s, waves);
        case 16:
        case 32: return launch_apply_mix_dst_mc(R, a, ntiles, s, waves);  // psgd_mixed_mfma.hip
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_flat_round_dst(const FlatArgs& a, const MixArgs& x, void* const* unc_dst, hipStream_t s) {
    if (a.nitems == 0) return hipSuccess;
    k_flat_round_dst<<<a.nitems, kBlock, 0, s>>>(a, x, unc_dst);
    return hipGetLastError();
}

}  // namespace psgd
