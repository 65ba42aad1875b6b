// Kernel instances of psgd_aggregate_comm_sgd and psgd_sgd_update (include/psgd.h; SgdDst, SgdArgs:
// psgd_internal.h). The fused ones are the destination-table final passes of psgd_apply_dst.hip
// (k_apply_dst, k_lowrank_dst: the same tiles, loads, LDS staging, MFMA sequence, fp32 arithmetic
// and residual store, so the average g of an element has the same bits) with the update forms of
// the tile bodies (kDstSgdVec / kDstSgdElem, psgd_stream.cuh): the n x m averages are never stored;
// at the element where they would have been, p and buf (loaded ahead of the tile's arithmetic)
// take the SGD update and are stored back. k_sgd_update is the element-wise kernel the fused form
// is defined against. All of them run sgd_update (psgd_stream.cuh), whose products are rounded on
// their own: the fused and the element-wise form agree bit for bit.
#include "psgd_final.cuh"
#include "psgd_sgd_flat.cuh"  // flat_sgd_item: the flat tail's update items

namespace psgd {

// The tile's momentum buffer and its tensor's record: workgroup-uniform loads, once per tile
__device__ __forceinline__ SgdTile sgd_tile(const SgdDst& x, int tensor) {
    SgdTile sg;
    sg.h = x.hyper[tensor];
    sg.buf = sg.h.momentum != 0.f ? static_cast<float*>(x.bufs[tensor]) : nullptr;
    return sg;
}

// true when the tile's first element (tensor base + row offset; with m % 4 == 0 every vector of
// the tile then) is 16-byte aligned in p and in buf. Workgroup-uniform: one test per tile.
__device__ __forceinline__ bool sgd_al16(const ApplyArgs& a, const SgdTile& sg, const MatDesc& d, const Tile& t) {
    const uintptr_t o = uintptr_t(int64_t(t.chunk) * d.chunk_rows * d.m) * sizeof(float);
    const uintptr_t p = reinterpret_cast<uintptr_t>(a.odst[d.tensor]) + o;
    const uintptr_t b = sg.buf ? reinterpret_cast<uintptr_t>(sg.buf) + o : 0;
    return ((p | b) & 15) == 0;
}

// k_apply_dst<R, NI, SHARED, false> with the update forms; the flat tail's update items lead
template <int R, int NI, bool SHARED>
__global__ __launch_bounds__(kBlock) void k_apply_sgd(ApplyArgs a, SgdDst x) {
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_sgd_item<kBlock>(a.flat, x, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const SgdTile sg = sgd_tile(x, d.tensor);
    if constexpr (R <= 8) {
        if (d.vec) {
            if (sgd_al16(a, sg, d, t))
                apply_tile<float, R, NI, SHARED, 4, false, float, kDstSgdVec>(a, d, t, &sg);
            else
                apply_tile<float, R, NI, SHARED, 4, false, float, kDstSgdElem>(a, d, t, &sg);
            return;
        }
    }
    if constexpr (R >= 16) {
        __shared__ __attribute__((aligned(16))) float qs[ApplyMfmaLds<R>::floats];
        constexpr int NS = SHARED ? 1 : 2;
        // k_apply_dst's choice between the matrix-core tile and its VALU fallback (they sum in
        // different orders): the gradients, the residual's destination and the plan's offset;
        // neither p nor buf enters it
        const uintptr_t rows = reinterpret_cast<uintptr_t>(a.grads[t.tensor]) |
                               reinterpret_cast<uintptr_t>(a.rdst ? a.rdst[d.tensor] : a.grads[t.tensor]) |
                               uintptr_t(d.out_off) * sizeof(float);
        if ((d.m & 3) == 0 && (rows & (4 * sizeof(float) - 1)) == 0 && a.nterms * NS <= kApplyMfmaSets) {
            if (sgd_al16(a, sg, d, t))
                apply_tile_mfma<float, R, SHARED, false, kDstSgdVec>(a, d, t, qs, &sg);
            else
                apply_tile_mfma<float, R, SHARED, false, kDstSgdElem>(a, d, t, qs, &sg);
            return;
        }
    }
    apply_tile<float, R, NI, SHARED, 1, false, float, kDstSgdVec>(a, d, t, &sg);
}

// k_lowrank_dst<R, NI> (the output pass after a fused k_final_odd) likewise
template <int R, int NI>
__global__ __launch_bounds__(kBlock) void k_lowrank_sgd(ApplyArgs a, SgdDst x) {
    static_assert(R <= 2, "k_final_odd's K-term form: rank buckets 1 and 2");
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_sgd_item<kBlock>(a.flat, x, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const SgdTile sg = sgd_tile(x, d.tensor);
    if (!d.vec)
        lowrank_tile<float, R, NI, 1, kDstSgdVec>(a, d, t, &sg);
    else if (sgd_al16(a, sg, d, t))
        lowrank_tile<float, R, NI, 4, kDstSgdVec>(a, d, t, &sg);
    else
        lowrank_tile<float, R, NI, 4, kDstSgdElem>(a, d, t, &sg);
}

// The element-wise update over a run table: one workgroup per item, at most kRunItem elements of
// one tensor from 64-bit element offset it.off. g, p and buf are 4-byte aligned independently.
// Where the item's three first addresses agree modulo 16 bytes (workgroup-uniform; the common
// case: whole tensors of the caching allocator) the item is a head of 0-3 elements up to the
// 16-byte boundary, 16-byte vectors and a tail; any other item runs as 4-byte accesses, one
// element per lane access. Every access goes through a descriptor of the item's own elements
// (past them: loads give zeros, stores are dropped), every load is issued before the first store.
__global__ __launch_bounds__(kBlock) void k_sgd_update(SgdArgs a) {
    const SgdItem it = a.items[blockIdx.x];
    const psgd_sgd_hyper h = a.hyper[it.tensor];
    const bool mom = h.momentum != 0.f;
    const float* gp = static_cast<const float*>(a.g[it.tensor]) + it.off;
    float* pp = static_cast<float*>(a.p[it.tensor]) + it.off;
    float* bp = mom ? static_cast<float*>(a.buf[it.tensor]) + it.off : nullptr;
    const uint32_t bytes = uint32_t(it.cnt) * 4u;
    const rsrc_t rG = make_rsrc(gp, bytes);
    const rsrc_t rP = make_rsrc(pp, bytes);
    const rsrc_t rB = make_rsrc(bp, mom ? bytes : 0u);
    const uint32_t ag = uint32_t(reinterpret_cast<uintptr_t>(gp)) & 15u, ap = uint32_t(reinterpret_cast<uintptr_t>(pp)) & 15u;
    const uint32_t ab = mom ? uint32_t(reinterpret_cast<uintptr_t>(bp)) & 15u : ap;
    if (ag == ap && ap == ab) {
        constexpr int PV = kRunItem / 4 / kBlock;  // vectors per thread
        const uint32_t head = ((16u - ag) & 15u) < bytes ? (16u - ag) & 15u : bytes;  // bytes before the boundary
        const uint32_t nvec = (bytes - head) / 16u;
        const uint32_t tail0 = head + nvec * 16u;  // the tail: bytes [tail0, bytes), at most 3 elements
        // the 0-3 head and 0-3 tail elements: lanes 0-2 and 3-5 of the workgroup
        const uint32_t e = threadIdx.x < 3 ? threadIdx.x * 4u : tail0 + (threadIdx.x - 3u) * 4u;
        const bool edge = threadIdx.x < 3 ? e < head : threadIdx.x < 6 && e < bytes;
        const uint32_t eo = edge ? e : kOob;
        float g[PV][4], p[PV][4], b[PV][4];
        float ge = BufIo<float>::ld1(rG, eo), pe = BufIo<float>::ld1(rP, eo), be = BufIo<float>::ld1(rB, eo);
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            const uint32_t v = uint32_t(q) * kBlock + threadIdx.x;
            const uint32_t off = v < nvec ? head + v * 16u : kOob;
            BufIo<float>::ld4(rG, off, g[q]);
            BufIo<float>::ld4(rP, off, p[q]);
            BufIo<float>::ld4(rB, off, b[q]);
        }
#pragma unroll
        for (int q = 0; q < PV; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                keep(g[q][c]);
                keep(p[q][c]);
                keep(b[q][c]);
            }
        keep(ge);
        keep(pe);
        keep(be);
        sgd_update(h, ge, pe, be);
        StIo<float>::st1<0>(rP, eo, pe);
        if (mom) StIo<float>::st1<0>(rB, eo, be);
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            const uint32_t v = uint32_t(q) * kBlock + threadIdx.x;
            const uint32_t off = v < nvec ? head + v * 16u : kOob;
#pragma unroll
            for (int c = 0; c < 4; ++c) sgd_update(h, g[q][c], p[q][c], b[q][c]);
            StIo<float>::st4<0>(rP, off, p[q]);
            if (mom) StIo<float>::st4<0>(rB, off, b[q]);
        }
        return;
    }
    constexpr int PER = kRunItem / kBlock;
    float g[PER], p[PER], b[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t off = (uint32_t(q) * kBlock + threadIdx.x) * 4u;  // < 16 KiB: past the item is out of range
        g[q] = BufIo<float>::ld1(rG, off);
        p[q] = BufIo<float>::ld1(rP, off);
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
        const uint32_t off = (uint32_t(q) * kBlock + threadIdx.x) * 4u;
        sgd_update(h, g[q], p[q], b[q]);
        StIo<float>::st1<0>(rP, off, p[q]);
        if (mom) StIo<float>::st1<0>(rB, off, b[q]);
    }
}

namespace {

template <typename F>
hipError_t ask_or_launch(F fn, int nblocks, hipStream_t s, int* waves, const ApplyArgs& a, const SgdDst& x) {
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    if (nblocks == 0) return hipSuccess;
    timed_launch(fn, dim3(nblocks), dim3(kBlock), s, a, x);
    return hipGetLastError();
}

// the instance dispatch_apply_dst<R> picks: the same NI and SHARED (the output's cache policy,
// ONT, has no update form: p' and buf' are stored plainly)
template <int R>
hipError_t dispatch_apply_sgd(int nterms, bool shared, const ApplyArgs& a, const SgdDst& x, int ntiles, hipStream_t s,
                              int* waves) {
    const int nb = ntiles + a.flat.nitems;
    auto go = [&](auto N) -> hipError_t {
        constexpr int NN = decltype(N)::value;
        if (shared) return ask_or_launch(&k_apply_sgd<R, NN, true>, nb, s, waves, a, x);
        return ask_or_launch(&k_apply_sgd<R, NN, false>, nb, s, waves, a, x);
    };
    if constexpr (R <= 8) return by_ni<1, 2, 3, 4>(apply_ni(R, nterms, shared), go);
    else return by_ni<>(-1, go);
}

template <int R>
hipError_t dispatch_lowrank_sgd(int nterms, const ApplyArgs& a, const SgdDst& x, int ntiles, hipStream_t s, int* waves) {
    return by_ni<1, 2, 4>(lowrank_ni(R, nterms), [&](auto N) -> hipError_t {
        return ask_or_launch(&k_lowrank_sgd<R, decltype(N)::value>, ntiles + a.flat.nitems, s, waves, a, x);
    });
}

}  // namespace

hipError_t launch_apply_sgd(int R, int nterms, bool shared, const ApplyArgs& a, const SgdDst& x, int ntiles,
                            hipStream_t s, int* waves) {
    switch (R) {
        case 1: return dispatch_apply_sgd<1>(nterms, shared, a, x, ntiles, s, waves);
        case 2: return dispatch_apply_sgd<2>(nterms, shared, a, x, ntiles, s, waves);
        case 4: return dispatch_apply_sgd<4>(nterms, shared, a, x, ntiles, s, waves);
        case 8: return dispatch_apply_sgd<8>(nterms, shared, a, x, ntiles, s, waves);
        case 16: return dispatch_apply_sgd<16>(nterms, shared, a, x, ntiles, s, waves);
        case 32: return dispatch_apply_sgd<32>(nterms, shared, a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_lowrank_sgd(int R, int nterms, const ApplyArgs& a, const SgdDst& x, int ntiles, hipStream_t s,
                              int* waves) {
    switch (R) {
        case 1: return dispatch_lowrank_sgd<1>(nterms, a, x, ntiles, s, waves);
        case 2: return dispatch_lowrank_sgd<2>(nterms, a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_sgd_update(const SgdArgs& a, hipStream_t s) {
    if (a.nitems <= 0) return hipSuccess;
    k_sgd_update<<<a.nitems, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace psgd
