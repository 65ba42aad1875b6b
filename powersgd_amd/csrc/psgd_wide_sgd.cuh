// The epilogue of the wide SGD passes (k_wide_apply_sgd, psgd_wide_sgd.hip; k_wide_apply_sgd_mp,
// psgd_wide_sgd_mp.hip): THE UPDATE of psgd_sgd_hyper on a 64 x 256 tile's elements from wide_pass's
// accumulators. The design notes are psgd_wide_sgd.hip's header.
#pragma once

#include "psgd_wide_pass.cuh"

namespace psgd {

namespace {

// steps of (p, buf) quads live at once with momentum; without, all kSteps of p
constexpr int kSgdRing = 3;

// the p (MOM: and buf) quads of one column step
template <bool MOM>
struct Pb {
    f32x4_t p[4];
    f32x4_t b[MOM ? 4 : 0];
};

// THE UPDATE on the tile's elements from the accumulators, and its stores. SHARED: the residual
// G - S is formed and stored here too (S is complete only now). MOM: the record's momentum != 0.
// MP (k_wide_apply_sgd_mp): P is the fp32 master weight and W its bf16 model tensor, which takes
// bf16(p') of the quad the p' store has just written: 8 bytes where m % 4 == 0 and W is 8-byte
// aligned (a test of its own, once per tile), else 2-byte pieces; store only, so it adds no quad
// to the ring.
template <bool SHARED, bool MOM, bool MP = false>
__device__ __forceinline__ void sgd_epilogue(const f32x4_t (&acc)[kSteps][4], const WideTile& w, float* __restrict__ G,
                                             bool gvec, float alpha, const psgd_sgd_hyper& h, float* __restrict__ P,
                                             float* __restrict__ B, bf16_t* __restrict__ W = nullptr) {
    constexpr int DEPTH = MOM ? kSgdRing : kSteps;
    psgd_sgd_hyper hh = h;
    if constexpr (!MOM) hh.momentum = 0.f;  // a constant here: sgd_update's buffer arithmetic is not compiled in
    const int kq = int(threadIdx.x & 63) >> 4;
    // one test per tile; the tile's first element is (row 64 chunk, column sbeg): with m % 4 == 0 a
    // multiple of four elements from the tensor's base, so the base's alignment is the tile's
    uintptr_t bases = reinterpret_cast<uintptr_t>(P);
    if constexpr (MOM) bases |= reinterpret_cast<uintptr_t>(B);
    const bool vec = w.m % 4 == 0 && (bases & 15) == 0;
    const bool wvec = MP && w.m % 4 == 0 && (reinterpret_cast<uintptr_t>(W) & 7) == 0;
    Pb<MOM> ring[DEPTH];
    auto request = [&](int s) {
        Pb<MOM>& x = ring[s % DEPTH];
        const int q4 = fresh(4 * kq);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t s4 = w.sbeg + 64 * s + 16 * u + q4;
            x.p[u] = ld_g4(P, w.n, w.m, w.o, s4, w.send, vec);
            if constexpr (MOM) x.b[u] = ld_g4(B, w.n, w.m, w.o, s4, w.send, vec);
        }
    };
#pragma unroll
    for (int s = 0; s < DEPTH - 1; ++s)
        if (s < w.nsteps) request(s);  // workgroup-uniform
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        if (s >= w.nsteps) continue;  // workgroup-uniform
        f32x4_t g[4];
        if constexpr (SHARED) {
            const int q4 = fresh(4 * kq);
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = ld_g4(G, w.n, w.m, w.o, w.sbeg + 64 * s + 16 * u + q4, w.send, gvec);
        }
        if (s + DEPTH - 1 < kSteps && s + DEPTH - 1 < w.nsteps) request(s + DEPTH - 1);  // into the slot step s - 1 left
        Pb<MOM>& c = ring[s % DEPTH];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t s4 = w.sbeg + 64 * s + 16 * u + fresh(4 * kq);
            if (s4 >= w.send) continue;
            f32x4_t avg;
            if constexpr (SHARED) {
                st_res4(G + w.o * w.m + s4, g[u] - acc[s][u], s4, w.send, gvec);
                avg = acc[s][u];
            } else {
                avg = acc[s][u] * alpha;
            }
            asm volatile("" : "+v"(avg));  // the average as k_wide_apply<float> stores it: a rounded value of its own
            f32x4_t pn = c.p[u], bn = {0.f, 0.f, 0.f, 0.f};
            if constexpr (MOM) bn = c.b[u];
            // elements past the tile's last column compute on zeros and store nothing
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pn[e], be = bn[e];
                sgd_update(hh, avg[e], pe, be);
                pn[e] = pe;
                bn[e] = be;
            }
            const int64_t at = w.o * w.m + s4;
            st_res4(P + at, pn, s4, w.send, vec);
            if constexpr (MOM) st_res4(B + at, bn, s4, w.send, vec);
            if constexpr (MP) st_out4(W + at, pn, s4, w.send, wvec);
        }
    }
}

}  // namespace

}  // namespace psgd
