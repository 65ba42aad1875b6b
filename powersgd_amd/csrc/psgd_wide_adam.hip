// The final pass of psgd_aggregate_comm_adam_wide and psgd_aggregate_mixed_comm_adam_wide
// (psgd_onecall.cpp): effective ranks 33-128, with the Adam / AdamW step applied where
// k_wide_apply<float> would have stored the fp32 average.
//
//   k_wide_apply_adam<R, SHARED, MP>   residual = G_0 - sum_k P_k Q_k^T (fp32, in place),
//                                      g = alpha sum_k Pbar_k Qbar_k^T, never stored:
//                                      (p, m, v) <- THE UPDATE(g, p, m, v); MP: w = bf16(p')
//
// Tile, accumulators, MFMA sequence and operand movement are k_wide_apply_mix's (wide_pass,
// psgd_wide_pass.cuh): the Q-side blocks staged once per workgroup in LDS (row stride R + 4 floats,
// two buffers, the next block's global loads ahead of the current MFMA chain, one barrier per
// block), the P side once per tile in registers. Every accumulator receives k_wide_apply<float>'s
// sequence, so the residual and g = acc x alpha (that kernel's one fp32 multiply; at world size 1
// the sums themselves) have its bits, and adam_update (psgd_stream.cuh) is the device function of
// k_adam_update / k_adam_update_mp: the fused step equals psgd_aggregate_comm followed by
// psgd_adam_update[_mp] bit for bit. g is pinned as a rounded value of its own before the update, so
// no product alpha x acc is contracted into the update's first add.
//
// The epilogue. A lane owns, per column step, four row quads (u = 0 .. 3) of its row: columns
// sbeg + 64 step + 16 u + 4 kq .. + 3. p, m and v are read at the same element of the tensor's own
// buffers (pointer tables indexed by MatDesc::tensor), updated and stored back; with MP the new
// weight, rounded to nearest even, also goes to the bf16 model tensor (store only).
//   access width   16 bytes where m % 4 == 0 and p, m and v are 16-byte aligned at the tile's first
//                  element (with m % 4 == 0 every quad of the tile then): one workgroup-uniform test
//                  per tile; else 4-byte element accesses. The bf16 store is 8 bytes where m % 4 == 0
//                  and w is 8-byte aligned, else 2 bytes; a test of its own. A quad that crosses the
//                  tile's last column runs element by element. No access leaves rows [0, n) x
//                  columns [sbeg, send) of the tensor: every one is predicated on its own index.
//   in flight      the p / m / v quads of one column step are 48 VGPRs. The requests of step s + 1
//                  are issued before the update and the stores of step s (vmcnt retires in order:
//                  waiting for them does not wait for those stores), so two steps' quads are live
//                  beside the 64 accumulator VGPRs; the P quads and the staging prefetch of the pass
//                  (up to 64 VGPRs at R = 128) are dead by then. None is requested while an LDS block
//                  is in flight: the first request follows the last pass. Addresses are formed at use
//                  (fresh()), none lives across a pass.
//   record         psgd_adam_hyper of the tile's tensor: nine dwords read once per tile from
//                  workgroup-uniform addresses; the decay branch and the lerp side are scalar.
// The flat tail's update items (psgd_adam_flat.cuh) lead the launch as workgroups blockIdx.x < nitems.
//
// LDS: 2 x 64 x (R + 4) floats = 34 816 / 67 584 bytes: two workgroups per CU at R = 128, which the
// register budget matches (two waves per SIMD, no scratch: profiles/adam_wide/resources.txt).
#include "psgd_adam_flat.cuh"
#include "psgd_wide_pass.cuh"

namespace psgd {

namespace {

// the tile's tensor: its parameter, moments, (MP) model tensor, record and access forms
struct WideAdamTile {
    float* p;
    float* m;
    float* v;
    bf16_t* w;
    psgd_adam_hyper h;
    bool vec, wvec;
};

// the p / m / v quads of one column step
struct Pmv {
    f32x4_t p[4], m[4], v[4];
};

__device__ __forceinline__ void ld_pmv(Pmv& x, const WideAdamTile& ad, const WideTile& w, int s) {
    const int q4 = fresh(4 * (int(threadIdx.x & 63) >> 4));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t s4 = w.sbeg + 64 * s + 16 * u + q4;
        x.p[u] = ld_g4(ad.p, w.n, w.m, w.o, s4, w.send, ad.vec);
        x.m[u] = ld_g4(ad.m, w.n, w.m, w.o, s4, w.send, ad.vec);
        x.v[u] = ld_g4(ad.v, w.n, w.m, w.o, s4, w.send, ad.vec);
    }
}

// THE UPDATE on one row quad from the average g, and its stores. Elements past the tile's last
// column compute on zeros (den = eps > 0) and store nothing.
template <bool MP>
__device__ __forceinline__ void adam_quad(const WideAdamTile& ad, const WideTile& w, int64_t s4, f32x4_t g, f32x4_t p,
                                          f32x4_t m, f32x4_t v) {
    if (s4 >= w.send) return;
    asm volatile("" : "+v"(g));  // the average as k_wide_apply<float> stores it: a rounded value of its own
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_update(ad.h, g[e], pe, me, ve);
        p[e] = pe;
        m[e] = me;
        v[e] = ve;
    }
    const int64_t at = w.o * w.m + s4;
    st_res4(ad.p + at, p, s4, w.send, ad.vec);
    st_res4(ad.m + at, m, s4, w.send, ad.vec);
    st_res4(ad.v + at, v, s4, w.send, ad.vec);
    if constexpr (MP) st_out4(ad.w + at, p, s4, w.send, ad.wvec);
}

}  // namespace

template <int R, bool SHARED, bool MP>
__global__ __launch_bounds__(kBlock, 2) void k_wide_apply_adam(WideArgs a, WideAdamDst x) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 64 * (R + 4)];
    const int nf = x.flat.nitems;
    if (int(blockIdx.x) < nf) {  // workgroup-uniform
        if constexpr (MP) flat_adam_mp_item<kBlock>(x.flat, x.y, blockIdx.x);
        else flat_adam_item<kBlock>(x.flat, x.y.x, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    const int kq = int(threadIdx.x & 63) >> 4;
    const WideTile w = wide_tile(t, d);
    float* __restrict__ G = static_cast<float*>(a.grads[t.tensor]);
    const bool gvec = w.m % 4 == 0 && reinterpret_cast<uintptr_t>(G) % 16 == 0;
    WideAdamTile ad;
    ad.p = static_cast<float*>(x.p[d.tensor]);
    ad.m = static_cast<float*>(x.y.x.ms[d.tensor]);
    ad.v = static_cast<float*>(x.y.x.vs[d.tensor]);
    ad.w = MP ? static_cast<bf16_t*>(x.y.ws[d.tensor]) : nullptr;
    ad.h = x.y.x.hyper[d.tensor];
    // the tile's first element is (row 64 chunk, column sbeg): with m % 4 == 0 a multiple of four
    // elements from the tensor's base, so the base's alignment is the tile's
    ad.vec = w.m % 4 == 0 && ((reinterpret_cast<uintptr_t>(ad.p) | reinterpret_cast<uintptr_t>(ad.m) |
                               reinterpret_cast<uintptr_t>(ad.v)) & 15) == 0;
    ad.wvec = MP && w.m % 4 == 0 && (reinterpret_cast<uintptr_t>(ad.w) & 7) == 0;

    f32x4_t acc[kSteps][4];
    if constexpr (SHARED) {
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[s][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        wide_pass<R, false>(acc, lds, a.res, a.nres, w);
    } else {
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[s][u] = ld_g4(G, w.n, w.m, w.o, w.sbeg + 64 * s + 16 * u + 4 * kq, w.send, gvec);
        wide_pass<R, true>(acc, lds, a.res, a.nres, w);  // reference powersgd.py:195-202
        if (w.ook) {
#pragma unroll
            for (int s = 0; s < kSteps; ++s)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t s4 = w.sbeg + 64 * s + 16 * u + fresh(4 * kq);
                    if (s4 < w.send) st_res4(G + w.o * w.m + s4, acc[s][u], s4, w.send, gvec);
                }
        }
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[s][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        wide_pass<R, false>(acc, lds, a.apx, a.nres, w);  // :211-219
    }
    if (!w.ook) return;  // past the last barrier
    const float alpha = a.alpha;
    Pmv pmv[2];
    ld_pmv(pmv[0], ad, w, 0);
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        if (s >= w.nsteps) continue;  // workgroup-uniform
        f32x4_t g[4];
        if constexpr (SHARED) {
            const int q4 = fresh(4 * kq);
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = ld_g4(G, w.n, w.m, w.o, w.sbeg + 64 * s + 16 * u + q4, w.send, gvec);
        }
        if (s + 1 < kSteps && s + 1 < w.nsteps) ld_pmv(pmv[(s + 1) & 1], ad, w, s + 1);
        const Pmv& c = pmv[s & 1];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t s4 = w.sbeg + 64 * s + 16 * u + fresh(4 * kq);
            if constexpr (SHARED) {
                if (s4 < w.send) st_res4(G + w.o * w.m + s4, g[u] - acc[s][u], s4, w.send, gvec);
                adam_quad<MP>(ad, w, s4, acc[s][u], c.p[u], c.m[u], c.v[u]);
            } else {
                adam_quad<MP>(ad, w, s4, acc[s][u] * alpha, c.p[u], c.m[u], c.v[u]);
            }
        }
    }
}

namespace {

template <int R, bool MP>
hipError_t wide_apply_adam(const WideArgs& a, const WideAdamDst& x, int ntiles, hipStream_t s, int* waves) {
    const auto fn = a.shared ? &k_wide_apply_adam<R, true, MP> : &k_wide_apply_adam<R, false, MP>;
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    const int nb = ntiles + x.flat.nitems;
    if (nb == 0) return hipSuccess;
    timed_launch(fn, dim3(nb), dim3(kBlock), s, a, x);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_wide_apply_adam(int R, bool mp, const WideArgs& a, const WideAdamDst& x, int ntiles, hipStream_t s,
                                  int* waves) {
    switch (R) {
        case 64: return mp ? wide_apply_adam<64, true>(a, x, ntiles, s, waves) : wide_apply_adam<64, false>(a, x, ntiles, s, waves);
        case 128: return mp ? wide_apply_adam<128, true>(a, x, ntiles, s, waves) : wide_apply_adam<128, false>(a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace psgd
