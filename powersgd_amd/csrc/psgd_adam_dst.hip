// Kernel instances of psgd_aggregate_comm_adam and psgd_adam_update (include/psgd.h; AdamDst,
// AdamArgs: psgd_internal.h). The fused ones are the destination-table final passes of
// psgd_apply_dst.hip (k_apply_dst, k_lowrank_dst: the same tiles, loads, LDS staging, MFMA sequence,
// fp32 arithmetic and residual store, so the average g of an element has the same bits) with the
// Adam forms of the tile bodies (kDstAdamVec / kDstAdamElem, psgd_stream.cuh): the n x m averages
// are never stored; at the element where they would have been, p, m and v take torch's Adam /
// AdamW update and are stored back. k_adam_update is the element-wise kernel the fused form is
// defined against. All of them run adam_update (psgd_stream.cuh), whose products are rounded on
// their own and whose sqrt and divisions are the correctly rounded ones: the fused and the
// element-wise form agree bit for bit.
//
// Data movement ("Fused Adam step"): p, m and v each have a buffer descriptor
// over the tile's rows of that tensor (12 SGPRs), and one 32-bit byte offset per vector serves all
// three and is formed again at the store, so no address lives across the term chain. The requests
// for all three go out ahead of a row's term chain (VALU tiles) or with the block's gradient quads
// ahead of the MFMA chain (matrix-core tiles); the VALU instances that cache their factor columns
// keep two rows in flight per lane instead of four where four would leave two waves per SIMD
// (adam_rows_in_flight).
#include "psgd_adam_flat.cuh"  // flat_adam_item: the flat tail's update items
#include "psgd_final.cuh"

namespace psgd {

// The tile's moments and its tensor's record: workgroup-uniform loads, once per tile
__device__ __forceinline__ AdamTile adam_tile(const AdamDst& x, int tensor) {
    AdamTile ad;
    ad.h = x.hyper[tensor];
    ad.m = static_cast<float*>(x.ms[tensor]);
    ad.v = static_cast<float*>(x.vs[tensor]);
    return ad;
}

// true when the tile's first element (tensor base + row offset; with m % 4 == 0 every vector of
// the tile then) is 16-byte aligned in p, m and v. Workgroup-uniform: one test per tile.
__device__ __forceinline__ bool adam_al16(const ApplyArgs& a, const AdamTile& ad, const MatDesc& d, const Tile& t) {
    const uintptr_t o = uintptr_t(int64_t(t.chunk) * d.chunk_rows * d.m) * sizeof(float);
    const uintptr_t p = reinterpret_cast<uintptr_t>(a.odst[d.tensor]) + o;
    const uintptr_t m = reinterpret_cast<uintptr_t>(ad.m) + o;
    const uintptr_t v = reinterpret_cast<uintptr_t>(ad.v) + o;
    return ((p | m | v) & 15) == 0;
}

// k_apply_dst<R, NI, SHARED, false> with the Adam forms; the flat tail's update items lead
template <int R, int NI, bool SHARED>
__global__ __launch_bounds__(kBlock) void k_apply_adam(ApplyArgs a, AdamDst x) {
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_adam_item<kBlock>(a.flat, x, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const AdamTile ad = adam_tile(x, d.tensor);
    if constexpr (R <= 8) {
        if (d.vec) {
            if (adam_al16(a, ad, d, t))
                apply_tile<float, R, NI, SHARED, 4, false, float, kDstAdamVec>(a, d, t, nullptr, &ad);
            else
                apply_tile<float, R, NI, SHARED, 4, false, float, kDstAdamElem>(a, d, t, nullptr, &ad);
            return;
        }
    }
    if constexpr (R >= 16) {
        __shared__ __attribute__((aligned(16))) float qs[ApplyMfmaLds<R>::floats];
        constexpr int NS = SHARED ? 1 : 2;
        // k_apply_dst's choice between the matrix-core tile and its VALU fallback (they sum in
        // different orders): the gradients, the residual's destination and the plan's offset;
        // none of p, m, v enters it
        const uintptr_t rows = reinterpret_cast<uintptr_t>(a.grads[t.tensor]) |
                               reinterpret_cast<uintptr_t>(a.rdst ? a.rdst[d.tensor] : a.grads[t.tensor]) |
                               uintptr_t(d.out_off) * sizeof(float);
        if ((d.m & 3) == 0 && (rows & (4 * sizeof(float) - 1)) == 0 && a.nterms * NS <= kApplyMfmaSets) {
            if (adam_al16(a, ad, d, t))
                apply_tile_mfma<float, R, SHARED, false, kDstAdamVec>(a, d, t, qs, nullptr, &ad);
            else
                apply_tile_mfma<float, R, SHARED, false, kDstAdamElem>(a, d, t, qs, nullptr, &ad);
            return;
        }
    }
    apply_tile<float, R, NI, SHARED, 1, false, float, kDstAdamVec>(a, d, t, nullptr, &ad);
}

// k_lowrank_dst<R, NI> (the output pass after a fused k_final_odd) likewise
template <int R, int NI>
__global__ __launch_bounds__(kBlock) void k_lowrank_adam(ApplyArgs a, AdamDst x) {
    static_assert(R <= 2, "k_final_odd's K-term form: rank buckets 1 and 2");
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_adam_item<kBlock>(a.flat, x, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const AdamTile ad = adam_tile(x, d.tensor);
    if (!d.vec)
        lowrank_tile<float, R, NI, 1, kDstAdamVec>(a, d, t, nullptr, &ad);
    else if (adam_al16(a, ad, d, t))
        lowrank_tile<float, R, NI, 4, kDstAdamVec>(a, d, t, nullptr, &ad);
    else
        lowrank_tile<float, R, NI, 4, kDstAdamElem>(a, d, t, nullptr, &ad);
}

// The element-wise update over a run table: one workgroup per item, at most kRunItem elements of
// one tensor from 64-bit element offset it.off. g, p, m and v are 4-byte aligned independently.
// Where the item's four first addresses agree modulo 16 bytes (workgroup-uniform; the common case:
// whole tensors of the caching allocator) the item is a head of 0-3 elements up to the 16-byte
// boundary, 16-byte vectors and a tail; any other item runs as 4-byte accesses, one element per
// lane access. Every access goes through a descriptor of the item's own elements (past them: loads
// give zeros, stores are dropped), every load is issued before the first store. A lane past the
// item's elements computes on zeros (den = eps > 0, or an inf / nan that is dropped with its store).
__global__ __launch_bounds__(kBlock) void k_adam_update(AdamArgs a) {
    const SgdItem it = a.items[blockIdx.x];
    const psgd_adam_hyper h = a.hyper[it.tensor];
    const float* gp = static_cast<const float*>(a.g[it.tensor]) + it.off;
    float* pp = static_cast<float*>(a.p[it.tensor]) + it.off;
    float* mp = static_cast<float*>(a.m[it.tensor]) + it.off;
    float* vp = static_cast<float*>(a.v[it.tensor]) + it.off;
    const uint32_t bytes = uint32_t(it.cnt) * 4u;
    const rsrc_t rG = make_rsrc(gp, bytes);
    const rsrc_t rP = make_rsrc(pp, bytes);
    const rsrc_t rM = make_rsrc(mp, bytes);
    const rsrc_t rV = make_rsrc(vp, bytes);
    const uint32_t ag = uint32_t(reinterpret_cast<uintptr_t>(gp)) & 15u, ap = uint32_t(reinterpret_cast<uintptr_t>(pp)) & 15u;
    const uint32_t am = uint32_t(reinterpret_cast<uintptr_t>(mp)) & 15u, av = uint32_t(reinterpret_cast<uintptr_t>(vp)) & 15u;
    if (ag == ap && ap == am && am == av) {
        constexpr int PV = kRunItem / 4 / kBlock;  // vectors per thread
        const uint32_t head = ((16u - ag) & 15u) < bytes ? (16u - ag) & 15u : bytes;  // bytes before the boundary
        const uint32_t nvec = (bytes - head) / 16u;
        const uint32_t tail0 = head + nvec * 16u;  // the tail: bytes [tail0, bytes), at most 3 elements
        // the 0-3 head and 0-3 tail elements: lanes 0-2 and 3-5 of the workgroup
        const uint32_t e = threadIdx.x < 3 ? threadIdx.x * 4u : tail0 + (threadIdx.x - 3u) * 4u;
        const bool edge = threadIdx.x < 3 ? e < head : threadIdx.x < 6 && e < bytes;
        const uint32_t eo = edge ? e : kOob;
        float g[PV][4], p[PV][4], m[PV][4], v[PV][4];
        float ge = BufIo<float>::ld1(rG, eo), pe = BufIo<float>::ld1(rP, eo), me = BufIo<float>::ld1(rM, eo),
              ve = BufIo<float>::ld1(rV, eo);
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            const uint32_t vi = uint32_t(q) * kBlock + threadIdx.x;
            const uint32_t off = vi < nvec ? head + vi * 16u : kOob;
            BufIo<float>::ld4(rG, off, g[q]);
            BufIo<float>::ld4(rP, off, p[q]);
            BufIo<float>::ld4(rM, off, m[q]);
            BufIo<float>::ld4(rV, off, v[q]);
        }
#pragma unroll
        for (int q = 0; q < PV; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                keep(g[q][c]);
                keep(p[q][c]);
                keep(m[q][c]);
                keep(v[q][c]);
            }
        keep(ge);
        keep(pe);
        keep(me);
        keep(ve);
        adam_update(h, ge, pe, me, ve);
        StIo<float>::st1<0>(rP, eo, pe);
        StIo<float>::st1<0>(rM, eo, me);
        StIo<float>::st1<0>(rV, eo, ve);
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            const uint32_t vi = uint32_t(q) * kBlock + threadIdx.x;
            const uint32_t off = vi < nvec ? head + vi * 16u : kOob;
#pragma unroll
            for (int c = 0; c < 4; ++c) adam_update(h, g[q][c], p[q][c], m[q][c], v[q][c]);
            StIo<float>::st4<0>(rP, off, p[q]);
            StIo<float>::st4<0>(rM, off, m[q]);
            StIo<float>::st4<0>(rV, off, v[q]);
        }
        return;
    }
    constexpr int PER = kRunItem / kBlock;
    float g[PER], p[PER], m[PER], v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t off = (uint32_t(q) * kBlock + threadIdx.x) * 4u;  // < 16 KiB: past the item is out of range
        g[q] = BufIo<float>::ld1(rG, off);
        p[q] = BufIo<float>::ld1(rP, off);
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
        const uint32_t off = (uint32_t(q) * kBlock + threadIdx.x) * 4u;
        adam_update(h, g[q], p[q], m[q], v[q]);
        StIo<float>::st1<0>(rP, off, p[q]);
        StIo<float>::st1<0>(rM, off, m[q]);
        StIo<float>::st1<0>(rV, off, v[q]);
    }
}

namespace {

template <typename F>
hipError_t ask_or_launch(F fn, int nblocks, hipStream_t s, int* waves, const ApplyArgs& a, const AdamDst& x) {
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    if (nblocks == 0) return hipSuccess;
    timed_launch(fn, dim3(nblocks), dim3(kBlock), s, a, x);
    return hipGetLastError();
}

// the instance dispatch_apply_dst<R> picks: the same NI and SHARED
template <int R>
hipError_t dispatch_apply_adam(int nterms, bool shared, const ApplyArgs& a, const AdamDst& x, int ntiles, hipStream_t s,
                               int* waves) {
    const int nb = ntiles + a.flat.nitems;
    auto go = [&](auto N) -> hipError_t {
        constexpr int NN = decltype(N)::value;
        if (shared) return ask_or_launch(&k_apply_adam<R, NN, true>, nb, s, waves, a, x);
        return ask_or_launch(&k_apply_adam<R, NN, false>, nb, s, waves, a, x);
    };
    if constexpr (R <= 8) return by_ni<1, 2, 3, 4>(apply_ni(R, nterms, shared), go);
    else return by_ni<>(-1, go);
}

template <int R>
hipError_t dispatch_lowrank_adam(int nterms, const ApplyArgs& a, const AdamDst& x, int ntiles, hipStream_t s, int* waves) {
    return by_ni<1, 2, 4>(lowrank_ni(R, nterms), [&](auto N) -> hipError_t {
        return ask_or_launch(&k_lowrank_adam<R, decltype(N)::value>, ntiles + a.flat.nitems, s, waves, a, x);
    });
}

}  // namespace

hipError_t launch_apply_adam(int R, int nterms, bool shared, const ApplyArgs& a, const AdamDst& x, int ntiles,
                             hipStream_t s, int* waves) {
    switch (R) {
        case 1: return dispatch_apply_adam<1>(nterms, shared, a, x, ntiles, s, waves);
        case 2: return dispatch_apply_adam<2>(nterms, shared, a, x, ntiles, s, waves);
        case 4: return dispatch_apply_adam<4>(nterms, shared, a, x, ntiles, s, waves);
        case 8: return dispatch_apply_adam<8>(nterms, shared, a, x, ntiles, s, waves);
        case 16: return dispatch_apply_adam<16>(nterms, shared, a, x, ntiles, s, waves);
        case 32: return dispatch_apply_adam<32>(nterms, shared, a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_lowrank_adam(int R, int nterms, const ApplyArgs& a, const AdamDst& x, int ntiles, hipStream_t s,
                               int* waves) {
    switch (R) {
        case 1: return dispatch_lowrank_adam<1>(nterms, a, x, ntiles, s, waves);
        case 2: return dispatch_lowrank_adam<2>(nterms, a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_adam_update(const AdamArgs& a, hipStream_t s) {
    if (a.nitems <= 0) return hipSuccess;
    k_adam_update<<<a.nitems, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace psgd
