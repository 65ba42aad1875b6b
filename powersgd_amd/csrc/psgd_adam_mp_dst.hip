// Kernel instances of psgd_aggregate_mixed_comm_adam and psgd_adam_update_mp (include/psgd.h;
// AdamMpDst, AdamMpArgs: psgd_internal.h): the Adam / AdamW step of a bf16 model with fp32 master
// weights and fp32 moments. The fused ones are the destination-table final passes of
// psgd_apply_dst.hip (k_apply_dst, k_lowrank_dst: the same tiles, loads, LDS staging, MFMA sequence,
// alpha x the accumulators and residual store, so the average g of an element has the same bits) on
// the fp32 residual, with the master-weight forms of the tile bodies (kDstAdamMpVec / kDstAdamMpElem,
// psgd_stream.cuh): at the element where the average would have been stored the master weight and
// both moments take THE UPDATE (adam_update, the only place it is written) and are stored back,
// and the new weight, rounded to bf16 as psgd_runs_gather rounds (bf16_pin_t: the fp32 value pinned,
// then round to nearest even), is stored at the model parameter's own address. No average, no
// master gradient and no master-to-model copy exists in memory. k_adam_update_mp is the element-wise
// kernel the form is defined against.
//
// Data movement: p, m and v as in psgd_adam_dst.hip (a descriptor each over the tile's rows, one
// shared 32-bit offset, requested ahead of the term / MFMA chain). The model tensor has a fourth
// descriptor over the same rows in 2-byte elements; it is only ever stored to, so it adds four SGPRs
// and no VGPR that lives across the chain: its offset is formed again at the store from the row and
// column the p' store used. A row quad's four bf16 weights leave as one 8-byte store where the tile
// is 8-byte aligned in w (and 16-byte in p, m, v), else as four 2-byte stores; one test per tile.
#include "psgd_adam_flat.cuh"  // flat_adam_mp_item: flat_adam_item plus the bf16 store
#include "psgd_final.cuh"

namespace psgd {

__device__ __forceinline__ AdamMpTile adam_mp_tile(const AdamMpDst& y, int tensor) {
    AdamMpTile ad;
    ad.h = y.x.hyper[tensor];
    ad.m = static_cast<float*>(y.x.ms[tensor]);
    ad.v = static_cast<float*>(y.x.vs[tensor]);
    ad.w = static_cast<uint16_t*>(y.ws[tensor]);
    return ad;
}

// true when the tile's first element (with m % 4 == 0 every row quad of the tile then) is 16-byte
// aligned in p, m and v and 8-byte aligned in w. Workgroup-uniform: one test per tile.
__device__ __forceinline__ bool adam_mp_vec(const ApplyArgs& a, const AdamMpTile& ad, const MatDesc& d, const Tile& t) {
    const uintptr_t e = uintptr_t(int64_t(t.chunk) * d.chunk_rows * d.m);
    const uintptr_t p = reinterpret_cast<uintptr_t>(a.odst[d.tensor]) + e * 4;
    const uintptr_t m = reinterpret_cast<uintptr_t>(ad.m) + e * 4;
    const uintptr_t v = reinterpret_cast<uintptr_t>(ad.v) + e * 4;
    const uintptr_t w = reinterpret_cast<uintptr_t>(ad.w) + e * 2;
    return ((p | m | v) & 15) == 0 && (w & 7) == 0;
}

// k_apply_dst<R, NI, SHARED, false> with the master-weight forms; the flat tail's update items lead
template <int R, int NI, bool SHARED>
__global__ __launch_bounds__(kBlock) void k_apply_adam_mp(ApplyArgs a, AdamMpDst y) {
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_adam_mp_item<kBlock>(a.flat, y, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const AdamMpTile ad = adam_mp_tile(y, d.tensor);
    if constexpr (R <= 8) {
        if (d.vec) {
            if (adam_mp_vec(a, ad, d, t))
                apply_tile<float, R, NI, SHARED, 4, false, float, kDstAdamMpVec>(a, d, t, nullptr, &ad);
            else
                apply_tile<float, R, NI, SHARED, 4, false, float, kDstAdamMpElem>(a, d, t, nullptr, &ad);
            return;
        }
    }
    if constexpr (R >= 16) {
        __shared__ __attribute__((aligned(16))) float qs[ApplyMfmaLds<R>::floats];
        constexpr int NS = SHARED ? 1 : 2;
        // k_apply_dst's choice between the matrix-core tile and its VALU fallback (they sum in
        // different orders): the gradients (here the residual views), the residual's destination
        // and the plan's offset; none of p, m, v, w enters it
        const uintptr_t rows = reinterpret_cast<uintptr_t>(a.grads[t.tensor]) |
                               reinterpret_cast<uintptr_t>(a.rdst ? a.rdst[d.tensor] : a.grads[t.tensor]) |
                               uintptr_t(d.out_off) * sizeof(float);
        if ((d.m & 3) == 0 && (rows & (4 * sizeof(float) - 1)) == 0 && a.nterms * NS <= kApplyMfmaSets) {
            if (adam_mp_vec(a, ad, d, t))
                apply_tile_mfma<float, R, SHARED, false, kDstAdamMpVec>(a, d, t, qs, nullptr, &ad);
            else
                apply_tile_mfma<float, R, SHARED, false, kDstAdamMpElem>(a, d, t, qs, nullptr, &ad);
            return;
        }
    }
    apply_tile<float, R, NI, SHARED, 1, false, float, kDstAdamMpVec>(a, d, t, nullptr, &ad);
}

// k_lowrank_dst<R, NI> (the output pass after a fused k_final_odd) likewise
template <int R, int NI>
__global__ __launch_bounds__(kBlock) void k_lowrank_adam_mp(ApplyArgs a, AdamMpDst y) {
    static_assert(R <= 2, "k_final_odd's K-term form: rank buckets 1 and 2");
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_adam_mp_item<kBlock>(a.flat, y, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const AdamMpTile ad = adam_mp_tile(y, d.tensor);
    if (!d.vec)
        lowrank_tile<float, R, NI, 1, kDstAdamMpVec>(a, d, t, nullptr, &ad);
    else if (adam_mp_vec(a, ad, d, t))
        lowrank_tile<float, R, NI, 4, kDstAdamMpVec>(a, d, t, nullptr, &ad);
    else
        lowrank_tile<float, R, NI, 4, kDstAdamMpElem>(a, d, t, nullptr, &ad);
}

// k_adam_update (psgd_adam_dst.hip) plus w[e] = bf16(p'[e]): one workgroup per item, at most
// kRunItem elements of one tensor from 64-bit element offset it.off. g, p, m and v are 4-byte
// aligned independently, w 2-byte. Where the item's four fp32 first addresses agree modulo 16 bytes
// and w is 8-byte aligned at the first 16-byte boundary of the others (workgroup-uniform) the item
// is a head of 0-3 elements, vectors (16 bytes of g, p, m, v; 8 bytes of w) and a tail; any other
// item runs as 4-byte accesses with 2-byte stores of w. Every access goes through a descriptor of
// the item's own elements (past them: loads give zeros, stores are dropped; w's offsets past the
// item are kOob by an explicit test), every load is issued before the first store.
__global__ __launch_bounds__(kBlock) void k_adam_update_mp(AdamMpArgs y) {
    const AdamArgs& a = y.a;
    const SgdItem it = a.items[blockIdx.x];
    const psgd_adam_hyper h = a.hyper[it.tensor];
    const float* gp = static_cast<const float*>(a.g[it.tensor]) + it.off;
    float* pp = static_cast<float*>(a.p[it.tensor]) + it.off;
    float* mp = static_cast<float*>(a.m[it.tensor]) + it.off;
    float* vp = static_cast<float*>(a.v[it.tensor]) + it.off;
    uint16_t* wp = static_cast<uint16_t*>(y.w[it.tensor]) + it.off;
    const uint32_t bytes = uint32_t(it.cnt) * 4u;
    const rsrc_t rG = make_rsrc(gp, bytes);
    const rsrc_t rP = make_rsrc(pp, bytes);
    const rsrc_t rM = make_rsrc(mp, bytes);
    const rsrc_t rV = make_rsrc(vp, bytes);
    const rsrc_t rW = make_rsrc(wp, bytes / 2u);
    const uint32_t ag = uint32_t(reinterpret_cast<uintptr_t>(gp)) & 15u, ap = uint32_t(reinterpret_cast<uintptr_t>(pp)) & 15u;
    const uint32_t am = uint32_t(reinterpret_cast<uintptr_t>(mp)) & 15u, av = uint32_t(reinterpret_cast<uintptr_t>(vp)) & 15u;
    const uint32_t head0 = (16u - ag) & 15u;  // bytes of g, p, m, v before their 16-byte boundary
    const uint32_t aw = (uint32_t(reinterpret_cast<uintptr_t>(wp)) + head0 / 2u) & 7u;
    if (ag == ap && ap == am && am == av && aw == 0u) {
        constexpr int PV = kRunItem / 4 / kBlock;  // vectors per thread
        const uint32_t head = head0 < bytes ? head0 : bytes;
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
        StIo<bf16_pin_t>::st1<0>(rW, edge ? e / 2u : kOob, pe);
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            const uint32_t vi = uint32_t(q) * kBlock + threadIdx.x;
            const bool in = vi < nvec;
            const uint32_t off = in ? head + vi * 16u : kOob;
#pragma unroll
            for (int c = 0; c < 4; ++c) adam_update(h, g[q][c], p[q][c], m[q][c], v[q][c]);
            StIo<float>::st4<0>(rP, off, p[q]);
            StIo<float>::st4<0>(rM, off, m[q]);
            StIo<float>::st4<0>(rV, off, v[q]);
            StIo<bf16_pin_t>::st4<0>(rW, in ? (head + vi * 16u) / 2u : kOob, p[q]);
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
        const uint32_t e = uint32_t(q) * kBlock + threadIdx.x;
        adam_update(h, g[q], p[q], m[q], v[q]);
        StIo<float>::st1<0>(rP, e * 4u, p[q]);
        StIo<float>::st1<0>(rM, e * 4u, m[q]);
        StIo<float>::st1<0>(rV, e * 4u, v[q]);
        StIo<bf16_pin_t>::st1<0>(rW, e < uint32_t(it.cnt) ? e * 2u : kOob, p[q]);
    }
}

namespace {

template <typename F>
hipError_t ask_or_launch(F fn, int nblocks, hipStream_t s, int* waves, const ApplyArgs& a, const AdamMpDst& y) {
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    if (nblocks == 0) return hipSuccess;
    timed_launch(fn, dim3(nblocks), dim3(kBlock), s, a, y);
    return hipGetLastError();
}

// the instance dispatch_apply_dst<R> picks: the same NI and SHARED
template <int R>
hipError_t dispatch_apply_adam_mp(int nterms, bool shared, const ApplyArgs& a, const AdamMpDst& y, int ntiles,
                                  hipStream_t s, int* waves) {
    const int nb = ntiles + a.flat.nitems;
    auto go = [&](auto N) -> hipError_t {
        constexpr int NN = decltype(N)::value;
        if (shared) return ask_or_launch(&k_apply_adam_mp<R, NN, true>, nb, s, waves, a, y);
        return ask_or_launch(&k_apply_adam_mp<R, NN, false>, nb, s, waves, a, y);
    };
    if constexpr (R <= 8) return by_ni<1, 2, 3, 4>(apply_ni(R, nterms, shared), go);
    else return by_ni<>(-1, go);
}

template <int R>
hipError_t dispatch_lowrank_adam_mp(int nterms, const ApplyArgs& a, const AdamMpDst& y, int ntiles, hipStream_t s,
                                    int* waves) {
    return by_ni<1, 2, 4>(lowrank_ni(R, nterms), [&](auto N) -> hipError_t {
        return ask_or_launch(&k_lowrank_adam_mp<R, decltype(N)::value>, ntiles + a.flat.nitems, s, waves, a, y);
    });
}

}  // namespace

hipError_t launch_apply_adam_mp(int R, int nterms, bool shared, const ApplyArgs& a, const AdamMpDst& y, int ntiles,
                                hipStream_t s, int* waves) {
    switch (R) {
        case 1: return dispatch_apply_adam_mp<1>(nterms, shared, a, y, ntiles, s, waves);
        case 2: return dispatch_apply_adam_mp<2>(nterms, shared, a, y, ntiles, s, waves);
        case 4: return dispatch_apply_adam_mp<4>(nterms, shared, a, y, ntiles, s, waves);
        case 8: return dispatch_apply_adam_mp<8>(nterms, shared, a, y, ntiles, s, waves);
        case 16: return dispatch_apply_adam_mp<16>(nterms, shared, a, y, ntiles, s, waves);
        case 32: return dispatch_apply_adam_mp<32>(nterms, shared, a, y, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_lowrank_adam_mp(int R, int nterms, const ApplyArgs& a, const AdamMpDst& y, int ntiles, hipStream_t s,
                                  int* waves) {
    switch (R) {
        case 1: return dispatch_lowrank_adam_mp<1>(nterms, a, y, ntiles, s, waves);
        case 2: return dispatch_lowrank_adam_mp<2>(nterms, a, y, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_adam_update_mp(const AdamMpArgs& y, hipStream_t s) {
    if (y.a.nitems <= 0) return hipSuccess;
    k_adam_update_mp<<<y.a.nitems, kBlock, 0, s>>>(y);
    return hipGetLastError();
}

}  // namespace psgd
