// Kernel instances of psgd_aggregate_mixed_comm_sgd and psgd_sgd_update_mp (include/psgd.h; SgdMpDst,
// SgdMpArgs: psgd_internal.h): the SGD step of a bf16 model with fp32 master weights and fp32
// momentum buffers. The fused ones are the destination-table final passes of psgd_apply_dst.hip
// (k_apply_dst, k_lowrank_dst: the same tiles, loads, LDS staging, MFMA sequence, alpha x the
// accumulators and residual store, so the average g of an element has the same bits) on the fp32
// residual, with the master-weight forms of the tile bodies (kDstSgdMpVec / kDstSgdMpElem,
// psgd_stream.cuh): at the element where the average would have been stored the master weight and
// the buffer take THE UPDATE (sgd_update, the only place it is written) and are stored back, and
// the new weight, rounded to bf16 as psgd_adam_update_mp rounds (bf16_pin_t: the fp32 value pinned,
// then round to nearest even), is stored at the model parameter's own address. No average, no
// master gradient and no master-to-model copy exists in memory: with momentum the pass moves
// 18 bytes per element (p and buf read; p', buf' and w written), without 10. k_sgd_update_mp is the
// element-wise kernel the form is defined against.
//
// Data movement: p and buf as in psgd_sgd_dst.hip (a descriptor each over the tile's rows, one
// shared 32-bit offset, requested ahead of the term / MFMA chain; a tensor without momentum has an
// empty buffer descriptor: no access). The model tensor has a third descriptor over the same rows in
// 2-byte elements; it is only ever stored to, so it adds four SGPRs and no VGPR that lives across
// the chain: its offset is formed again at the store from the row and column the p' store used. A
// row quad's four bf16 weights leave as one 8-byte store where the tile is 8-byte aligned in w (and
// 16-byte in p and buf), else as four 2-byte stores; one test per tile.
#include "psgd_final.cuh"
#include "psgd_sgd_flat.cuh"  // flat_sgd_mp_item: flat_sgd_item plus the bf16 store

namespace psgd {

// The tile's buffer, model tensor and record: workgroup-uniform loads, once per tile
__device__ __forceinline__ SgdMpTile sgd_mp_tile(const SgdMpDst& y, int tensor) {
    SgdMpTile sg;
    sg.h = y.x.hyper[tensor];
    sg.buf = sg.h.momentum != 0.f ? static_cast<float*>(y.x.bufs[tensor]) : nullptr;
    sg.w = static_cast<uint16_t*>(y.ws[tensor]);
    return sg;
}

// true when the tile's first element (with m % 4 == 0 every row quad of the tile then) is 16-byte
// aligned in p and (with momentum) buf and 8-byte aligned in w. Workgroup-uniform: one test per tile.
__device__ __forceinline__ bool sgd_mp_vec(const ApplyArgs& a, const SgdMpTile& sg, const MatDesc& d, const Tile& t) {
    const uintptr_t e = uintptr_t(int64_t(t.chunk) * d.chunk_rows * d.m);
    const uintptr_t p = reinterpret_cast<uintptr_t>(a.odst[d.tensor]) + e * 4;
    const uintptr_t b = sg.buf ? reinterpret_cast<uintptr_t>(sg.buf) + e * 4 : 0;
    const uintptr_t w = reinterpret_cast<uintptr_t>(sg.w) + e * 2;
    return ((p | b) & 15) == 0 && (w & 7) == 0;
}

// k_apply_dst<R, NI, SHARED, false> with the master-weight forms; the flat tail's update items lead
template <int R, int NI, bool SHARED>
__global__ __launch_bounds__(kBlock) void k_apply_sgd_mp(ApplyArgs a, SgdMpDst y) {
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_sgd_mp_item<kBlock>(a.flat, y, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const SgdMpTile sg = sgd_mp_tile(y, d.tensor);
    if constexpr (R <= 8) {
        if (d.vec) {
            if (sgd_mp_vec(a, sg, d, t))
                apply_tile<float, R, NI, SHARED, 4, false, float, kDstSgdMpVec>(a, d, t, &sg);
            else
                apply_tile<float, R, NI, SHARED, 4, false, float, kDstSgdMpElem>(a, d, t, &sg);
            return;
        }
    }
    if constexpr (R >= 16) {
        __shared__ __attribute__((aligned(16))) float qs[ApplyMfmaLds<R>::floats];
        constexpr int NS = SHARED ? 1 : 2;
        // k_apply_dst's choice between the matrix-core tile and its VALU fallback (they sum in
        // different orders): the gradients (here the residual views), the residual's destination
        // and the plan's offset; none of p, buf, w enters it
        const uintptr_t rows = reinterpret_cast<uintptr_t>(a.grads[t.tensor]) |
                               reinterpret_cast<uintptr_t>(a.rdst ? a.rdst[d.tensor] : a.grads[t.tensor]) |
                               uintptr_t(d.out_off) * sizeof(float);
        if ((d.m & 3) == 0 && (rows & (4 * sizeof(float) - 1)) == 0 && a.nterms * NS <= kApplyMfmaSets) {
            if (sgd_mp_vec(a, sg, d, t))
                apply_tile_mfma<float, R, SHARED, false, kDstSgdMpVec>(a, d, t, qs, &sg);
            else
                apply_tile_mfma<float, R, SHARED, false, kDstSgdMpElem>(a, d, t, qs, &sg);
            return;
        }
    }
    apply_tile<float, R, NI, SHARED, 1, false, float, kDstSgdMpVec>(a, d, t, &sg);
}

// k_lowrank_dst<R, NI> (the output pass after a fused k_final_odd) likewise
template <int R, int NI>
__global__ __launch_bounds__(kBlock) void k_lowrank_sgd_mp(ApplyArgs a, SgdMpDst y) {
    static_assert(R <= 2, "k_final_odd's K-term form: rank buckets 1 and 2");
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_sgd_mp_item<kBlock>(a.flat, y, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const SgdMpTile sg = sgd_mp_tile(y, d.tensor);
    if (!d.vec)
        lowrank_tile<float, R, NI, 1, kDstSgdMpVec>(a, d, t, &sg);
    else if (sgd_mp_vec(a, sg, d, t))
        lowrank_tile<float, R, NI, 4, kDstSgdMpVec>(a, d, t, &sg);
    else
        lowrank_tile<float, R, NI, 4, kDstSgdMpElem>(a, d, t, &sg);
}

// k_sgd_update (psgd_sgd_dst.hip) plus w[e] = bf16(p'[e]): one workgroup per item, at most kRunItem
// elements of one tensor from 64-bit element offset it.off. g, p and buf are 4-byte aligned
// independently, w 2-byte. Where the item's fp32 first addresses (g, p; with momentum: buf) agree
// modulo 16 bytes and w is 8-byte aligned at the first 16-byte boundary of the others
// (workgroup-uniform) the item is a head of 0-3 elements, vectors (16 bytes of g, p, buf; 8 bytes of
// w) and a tail; any other item runs as 4-byte accesses with 2-byte stores of w. Every access goes
// through a descriptor of the item's own elements (past them: loads give zeros, stores are dropped;
// w's offsets past the item are kOob by an explicit test; the buffer's descriptor is empty without
// momentum), every load is issued before the first store.
__global__ __launch_bounds__(kBlock) void k_sgd_update_mp(SgdMpArgs y) {
    const SgdArgs& a = y.a;
    const SgdItem it = a.items[blockIdx.x];
    const psgd_sgd_hyper h = a.hyper[it.tensor];
    const bool mom = h.momentum != 0.f;
    const float* gp = static_cast<const float*>(a.g[it.tensor]) + it.off;
    float* pp = static_cast<float*>(a.p[it.tensor]) + it.off;
    float* bp = mom ? static_cast<float*>(a.buf[it.tensor]) + it.off : nullptr;
    uint16_t* wp = static_cast<uint16_t*>(y.w[it.tensor]) + it.off;
    const uint32_t bytes = uint32_t(it.cnt) * 4u;
    const rsrc_t rG = make_rsrc(gp, bytes);
    const rsrc_t rP = make_rsrc(pp, bytes);
    const rsrc_t rB = make_rsrc(bp, mom ? bytes : 0u);
    const rsrc_t rW = make_rsrc(wp, bytes / 2u);
    const uint32_t ag = uint32_t(reinterpret_cast<uintptr_t>(gp)) & 15u, ap = uint32_t(reinterpret_cast<uintptr_t>(pp)) & 15u;
    const uint32_t ab = mom ? uint32_t(reinterpret_cast<uintptr_t>(bp)) & 15u : ap;
    const uint32_t head0 = (16u - ag) & 15u;  // bytes of g, p, buf before their 16-byte boundary
    const uint32_t aw = (uint32_t(reinterpret_cast<uintptr_t>(wp)) + head0 / 2u) & 7u;
    if (ag == ap && ap == ab && aw == 0u) {
        constexpr int PV = kRunItem / 4 / kBlock;  // vectors per thread
        const uint32_t head = head0 < bytes ? head0 : bytes;
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
            const uint32_t vi = uint32_t(q) * kBlock + threadIdx.x;
            const uint32_t off = vi < nvec ? head + vi * 16u : kOob;
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
        StIo<bf16_pin_t>::st1<0>(rW, edge ? e / 2u : kOob, pe);
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            const uint32_t vi = uint32_t(q) * kBlock + threadIdx.x;
            const bool in = vi < nvec;
            const uint32_t off = in ? head + vi * 16u : kOob;
#pragma unroll
            for (int c = 0; c < 4; ++c) sgd_update(h, g[q][c], p[q][c], b[q][c]);
            StIo<float>::st4<0>(rP, off, p[q]);
            if (mom) StIo<float>::st4<0>(rB, off, b[q]);
            StIo<bf16_pin_t>::st4<0>(rW, in ? (head + vi * 16u) / 2u : kOob, p[q]);
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
        const uint32_t e = uint32_t(q) * kBlock + threadIdx.x;
        sgd_update(h, g[q], p[q], b[q]);
        StIo<float>::st1<0>(rP, e * 4u, p[q]);
        if (mom) StIo<float>::st1<0>(rB, e * 4u, b[q]);
        StIo<bf16_pin_t>::st1<0>(rW, e < uint32_t(it.cnt) ? e * 2u : kOob, p[q]);
    }
}

namespace {

template <typename F>
hipError_t ask_or_launch(F fn, int nblocks, hipStream_t s, int* waves, const ApplyArgs& a, const SgdMpDst& y) {
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    if (nblocks == 0) return hipSuccess;
    timed_launch(fn, dim3(nblocks), dim3(kBlock), s, a, y);
    return hipGetLastError();
}

// the instance dispatch_apply_dst<R> picks: the same NI and SHARED
template <int R>
hipError_t dispatch_apply_sgd_mp(int nterms, bool shared, const ApplyArgs& a, const SgdMpDst& y, int ntiles,
                                 hipStream_t s, int* waves) {
    const int nb = ntiles + a.flat.nitems;
    auto go = [&](auto N) -> hipError_t {
        constexpr int NN = decltype(N)::value;
        if (shared) return ask_or_launch(&k_apply_sgd_mp<R, NN, true>, nb, s, waves, a, y);
        return ask_or_launch(&k_apply_sgd_mp<R, NN, false>, nb, s, waves, a, y);
    };
    if constexpr (R <= 8) return by_ni<1, 2, 3, 4>(apply_ni(R, nterms, shared), go);
    else return by_ni<>(-1, go);
}

template <int R>
hipError_t dispatch_lowrank_sgd_mp(int nterms, const ApplyArgs& a, const SgdMpDst& y, int ntiles, hipStream_t s,
                                   int* waves) {
    return by_ni<1, 2, 4>(lowrank_ni(R, nterms), [&](auto N) -> hipError_t {
        return ask_or_launch(&k_lowrank_sgd_mp<R, decltype(N)::value>, ntiles + a.flat.nitems, s, waves, a, y);
    });
}

}  // namespace

hipError_t launch_apply_sgd_mp(int R, int nterms, bool shared, const ApplyArgs& a, const SgdMpDst& y, int ntiles,
                               hipStream_t s, int* waves) {
    switch (R) {
        case 1: return dispatch_apply_sgd_mp<1>(nterms, shared, a, y, ntiles, s, waves);
        case 2: return dispatch_apply_sgd_mp<2>(nterms, shared, a, y, ntiles, s, waves);
        case 4: return dispatch_apply_sgd_mp<4>(nterms, shared, a, y, ntiles, s, waves);
        case 8: return dispatch_apply_sgd_mp<8>(nterms, shared, a, y, ntiles, s, waves);
        case 16: return dispatch_apply_sgd_mp<16>(nterms, shared, a, y, ntiles, s, waves);
        case 32: return dispatch_apply_sgd_mp<32>(nterms, shared, a, y, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_lowrank_sgd_mp(int R, int nterms, const ApplyArgs& a, const SgdMpDst& y, int ntiles, hipStream_t s,
                                 int* waves) {
    switch (R) {
        case 1: return dispatch_lowrank_sgd_mp<1>(nterms, a, y, ntiles, s, waves);
        case 2: return dispatch_lowrank_sgd_mp<2>(nterms, a, y, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_sgd_update_mp(const SgdMpArgs& y, hipStream_t s) {
    if (y.a.nitems <= 0) return hipSuccess;
    k_sgd_update_mp<<<y.a.nitems, kBlock, 0, s>>>(y);
    return hipGetLastError();
}

}  // namespace psgd
