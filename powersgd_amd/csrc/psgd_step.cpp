// Step drivers behind the C ABI of include/psgd.h: one power iteration (compress) and the output
// pass (decompress) for fp32/bf16 and fp64 plans, psgd_aggregate and its flat / communicator
// variants, and the reducer building blocks.
#include <cstdio>
#include <cstdlib>

#include "psgd_plan.h"

namespace psgd {

thread_local const KernelTiming* g_kernel_timing = nullptr;

// dtype dispatch of the per-dtype launchers (a plan is fp32 or bf16 here; fp64 has its own)
#define BY_DTYPE(fn, ...) (dtype == PSGD_F32 ? fn##_f32(__VA_ARGS__) : fn##_bf16(__VA_ARGS__))
hipError_t launch_final_oe(int dtype, int nres, int smax, const FinalArgs& a, int ntiles, hipStream_t s, int* waves) {
    return BY_DTYPE(launch_final_oe, nres, smax, a, ntiles, s, waves);
}
hipError_t launch_final_odd(int dtype, int R, int nres, int smax, const FinalArgs& a, int ntiles,
                            hipStream_t s, int* waves) {
    return BY_DTYPE(launch_final_odd, R, nres, smax, a, ntiles, s, waves);
}
hipError_t launch_lowrank_out(int dtype, int R, int nterms, const ApplyArgs& a, int ntiles, hipStream_t s) {
    return BY_DTYPE(launch_lowrank_out, R, nterms, a, ntiles, s);
}
hipError_t launch_odd_mfma(int dtype, int R, int nres, const ProductArgs& a, int ntiles, hipStream_t s) {
    return BY_DTYPE(launch_odd_mfma, R, nres, a, ntiles, s);
}
hipError_t launch_even(int dtype, int R, int nres, const ProductArgs& a, int nwg, hipStream_t s) {
    return BY_DTYPE(launch_even, R, nres, a, nwg, s);
}
hipError_t launch_product_odd(int dtype, int R, int nres, const ProductArgs& a, int ntiles, hipStream_t s) {
    return BY_DTYPE(launch_product_odd, R, nres, a, ntiles, s);
}
hipError_t launch_apply(int dtype, int R, int nterms, bool shared, const ApplyArgs& a, int ntiles, hipStream_t s) {
    return BY_DTYPE(launch_apply, R, nterms, shared, a, ntiles, s);
}
#undef BY_DTYPE

// Select (or upload, stream-ordered) the gradient pointer table; switch matrices whose
// gradient is not vector-aligned to the scalar path (rare: views into unaligned flat buffers;
// only that re-tiling synchronises, because the tile tables are rewritten in place).
int refresh_pointers(psgd_plan* p, void* const* grads, hipStream_t stream) {
    const size_t nt = p->shapes.size();
    for (size_t i = 0; i < nt; ++i)
        if (!grads[i]) return fail(PSGD_ERR_VALUE, "null gradient pointer");
    if (p->wide()) {  // the wide kernels test each gradient's alignment themselves: no re-tiling
        PSGD_HIP(p->grad_tab.select(grads, stream));
        return PSGD_OK;
    }
    const uintptr_t need = p->dtype == PSGD_F32 ? 16 : 8;
    bool same_vec = true;
    for (size_t i = 0; same_vec && i < p->mats.size(); ++i)
        same_vec = p->vec_now[i] == int(p->base_vec[i] && (reinterpret_cast<uintptr_t>(grads[p->mats[i].tensor]) % need == 0));
    if (!same_vec) {
        std::vector<int> vec(p->mats.size());
        for (size_t i = 0; i < p->mats.size(); ++i)
            vec[i] = p->base_vec[i] && (reinterpret_cast<uintptr_t>(grads[p->mats[i].tensor]) % need == 0);
        PSGD_HIP(hipStreamSynchronize(stream));  // earlier launches may still read the tile tables
        p->set_vec(vec);
        if (int st = p->upload_tiles()) return st;
    }
    PSGD_HIP(p->grad_tab.select(grads, stream));
    return PSGD_OK;
}

}  // namespace psgd

namespace {

void fill_terms(const psgd_plan* p, int64_t step, int count, Terms& res) {
    for (int j = 0; j < count; ++j) {
        const bool e = p->even(step, j);
        // local rank-r term of iteration j: even -> (P_j = X_j, Q_j = Y_j); odd -> (P_j = Y_j, Q_j = X_j)
        res.p[j] = e ? p->hist(0, j) : p->hist(1, j);
        res.q[j] = e ? p->hist(1, j) : p->hist(0, j);
    }
    for (int j = count; j < kMaxTerms; ++j) res.p[j] = res.q[j] = nullptr;
}

// Timing (benchmarks): HIP events of the final pass (k_apply, or the fused final odd kernel):
// recorded by the kernel's own dispatch (timed_launch) for the fp32/bf16 kernels (`direct`), or
// around the launch on its stream (fp64 apply).
struct TimedScope {
    KernelTiming kt{};
    explicit TimedScope(const std::pair<hipEvent_t, hipEvent_t>* ev) {
        if (ev) {
            kt = KernelTiming{ev->first, ev->second};
            g_kernel_timing = &kt;
        }
    }
    ~TimedScope() { g_kernel_timing = nullptr; }
};
int timing_begin(psgd_plan* p, hipStream_t s, std::pair<hipEvent_t, hipEvent_t>** ev, bool direct) {
    *ev = nullptr;
    if (!p->timing) return PSGD_OK;
    if (p->ev_used == p->ev_pool.size()) {
        std::pair<hipEvent_t, hipEvent_t> e;
        // no system-scope fence: a system-scope release writes back the L2s around the timed
        // kernel (~5.6 us of idle queue per event in the traces) that a plain step never pays
        PSGD_HIP(hipEventCreateWithFlags(&e.first, hipEventDisableSystemFence));
        PSGD_HIP(hipEventCreateWithFlags(&e.second, hipEventDisableSystemFence));
        p->ev_pool.push_back(e);
    }
    *ev = &p->ev_pool[p->ev_used++];
    if (!direct) PSGD_HIP(hipEventRecord((*ev)->first, s));
    return PSGD_OK;
}

// ---------------------------------------------------------------- fp64 plans ------
// The same iteration structure as the fp32 path below, on psgd_f64.hip's kernels: orthonormalise
// the in-factor (saving the all-reduced values of the previous iteration), product with
// G_k formed on the fly, and for even iterations the fixed-order partial reduction.
void fill_terms64(const psgd_plan* p, int64_t step, int count, TermsF64& res) {
    for (int j = 0; j < count; ++j) {
        const bool e = p->even(step, j);
        res.p[j] = e ? p->hist64(0, j) : p->hist64(1, j);
        res.q[j] = e ? p->hist64(1, j) : p->hist64(0, j);
    }
    for (int j = count; j < kMaxTerms; ++j) res.p[j] = res.q[j] = nullptr;
}

int compress_f64(psgd_plan* p, void* const* grads, int64_t step, int32_t it, hipStream_t s) {
    if (int st = refresh_pointers(p, grads, s)) return st;
    const bool even = p->even(step, it);
    double* P = reinterpret_cast<double*>(p->P);
    double* Q = reinterpret_cast<double*>(p->Q);
    double* in = even ? P : Q;
    double* out = even ? Q : P;
    F64OrthArgs oa{};
    oa.units = p->dev(even ? p->units_p : p->units_q);
    oa.state = in;
    oa.hx = p->hist64(0, it);
    oa.save = it > 0 ? p->hist64(2, it - 1) : nullptr;  // keep the all-reduced factor of it-1
    PSGD_HIP(launch_f64_orth(p->rbucket, oa, int(even ? p->units_p.size() : p->units_q.size()), s));
    F64Args a{};
    a.mats = p->dev(p->mats);
    a.grads = p->grad_tab.table();
    a.x = p->hist64(0, it);
    a.part = p->dev<double>(p->o_f64_part);
    a.part_off = p->dev(p->f64_part_off);
    a.y = out;
    a.yh = p->hist64(1, it);
    fill_terms64(p, step, it, a.res);
    a.nres = it;
    if (even) {
        a.tiles = p->dev(p->f64_even);
        PSGD_HIP(launch_f64_product(true, p->rbucket, a, int(p->f64_even.size()), s));
        a.items = p->dev(p->red_even);
        PSGD_HIP(launch_f64_reduce(p->rbucket, a, int(p->red_even.size()), s));
    } else {
        a.tiles = p->dev(p->f64_odd);
        PSGD_HIP(launch_f64_product(false, p->rbucket, a, int(p->f64_odd.size()), s));
    }
    return PSGD_OK;
}

int decompress_f64(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world, hipStream_t s) {
    if (int st = refresh_pointers(p, grads, s)) return st;
    const int I = p->iters;
    F64Args a{};
    a.mats = p->dev(p->mats);
    a.tiles = p->dev(p->f64_apply);
    a.grads = p->grad_tab.table();
    a.out = out;
    fill_terms64(p, step, I, a.res);
    double* last = reinterpret_cast<double*>(p->even(step, I - 1) ? p->Q : p->P);
    for (int k = 0; k < I; ++k) {
        const bool e = p->even(step, k);
        double* ybar = k + 1 < I ? p->hist64(2, k) : last;  // all-reduced factor of iteration k
        a.apx.p[k] = e ? p->hist64(0, k) : ybar;
        a.apx.q[k] = e ? ybar : p->hist64(0, k);
    }
    a.nres = I;
    a.alpha = 1.0 / double(world);  // reference alpha = 1 / num_workers (:218)
    std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
    if (int st = timing_begin(p, s, &ev, false)) return st;
    PSGD_HIP(launch_f64_apply(p->rbucket, a, int(p->f64_apply.size()), s));
    if (ev) PSGD_HIP(hipEventRecord(ev->second, s));
    return PSGD_OK;
}

// ---------------------------------------------------------------- wide plans ------
// Effective ranks 33-128 (psgd_wide.hip), the fp64 pair's structure on fp32 factors:
// orthonormalise the in-factor (Cholesky-QR in three launches; the all-reduced factor of the
// previous iteration goes to history slot 2, the orthonormal one to slot 0), the product with
// G_k formed on the matrix core, then the fixed-order partial reduction (both parities: the odd
// product is split over column strips as well). psgd_compress never writes the gradients.
int compress_wide(psgd_plan* p, void* const* grads, int64_t step, int32_t it, hipStream_t s) {
    if (int st = refresh_pointers(p, grads, s)) return st;
    const bool even = p->even(step, it);
    WideOrthArgs oa{};
    oa.units = p->dev(even ? p->units_p : p->units_q);
    oa.items = p->dev(even ? p->wide_gp : p->wide_gq);
    oa.slot0 = p->dev(even ? p->wide_slot_p : p->wide_slot_q);
    oa.state = even ? p->P : p->Q;
    oa.hx = p->hist(0, it);
    oa.save = it > 0 ? p->hist(2, it - 1) : nullptr;  // keep the all-reduced factor of it-1
    oa.gram = p->dev<double>(p->o_wide_gram);
    oa.m = p->dev<double>(p->o_wide_m);
    oa.sg = p->dev<double>(p->o_wide_sg);
    oa.ok = p->dev<int32_t>(p->o_wide_ok);
    const int nunits = int(even ? p->units_p.size() : p->units_q.size());
    PSGD_HIP(launch_wide_orth(p->rbucket, oa, nunits, int(even ? p->wide_gp.size() : p->wide_gq.size()), s));
    WideArgs a{};
    a.mats = p->dev(p->mats);
    a.tiles = p->dev(even ? p->wide_even : p->wide_odd);
    a.grads = p->grad_tab.table();
    a.x = p->hist(0, it);
    a.part = p->dev<float>(p->o_wide_part);
    fill_terms(p, step, it, a.res);
    a.nres = it;
    a.y = even ? p->Q : p->P;
    a.yh = p->hist(1, it);
    a.items = p->dev(even ? p->red_even : p->red_odd);
    a.even = even ? 1 : 0;
    PSGD_HIP(launch_wide_product(p->dtype, p->rbucket, even, a, int(even ? p->wide_even.size() : p->wide_odd.size()), s));
    PSGD_HIP(launch_wide_reduce(a, int(even ? p->red_even.size() : p->red_odd.size()), s));
    return PSGD_OK;
}

int decompress_wide(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world, hipStream_t s) {
    if (int st = refresh_pointers(p, grads, s)) return st;
    const int I = p->iters;
    WideArgs a{};
    a.mats = p->dev(p->mats);
    a.tiles = p->dev(p->wide_apply);
    a.grads = p->grad_tab.table();
    a.out = out;
    fill_terms(p, step, I, a.res);
    float* last = p->even(step, I - 1) ? p->Q : p->P;  // all-reduced factor of the last iteration
    for (int k = 0; k < kMaxTerms; ++k) a.apx.p[k] = a.apx.q[k] = nullptr;
    for (int k = 0; k < I; ++k) {
        const bool e = p->even(step, k);
        float* ybar = k + 1 < I ? p->hist(2, k) : last;
        a.apx.p[k] = e ? p->hist(0, k) : ybar;
        a.apx.q[k] = e ? ybar : p->hist(0, k);
    }
    a.nres = I;
    a.alpha = float(1.0 / double(world));  // reference alpha = 1 / num_workers (:218)
    a.shared = world == 1 ? 1 : 0;         // the all-reduced factors are the local ones
    std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
    if (int st = timing_begin(p, s, &ev, true)) return st;
    TimedScope ts(ev);
    PSGD_HIP(launch_wide_apply(p->dtype, p->rbucket, a, int(p->wide_apply.size()), s));
    return PSGD_OK;
}

int refuse_wide(const psgd_plan* p, const char* what) {
    if (!p->wide()) return PSGD_OK;
    return fail(PSGD_ERR_VALUE, std::string(what) + ": ranks above 32 are not supported there");
}

// Diagnostic (PSGD_EVEN_STAMPS=<file>, with a library built -DPSGD_EVEN_STAMPS): after every
// k_even launch, synchronise and append its per-workgroup stamps to <file>: one line per launch,
// "nwg", then per workgroup its segments' gradient bytes and the kEvenStamps words
// (tools/even_stamps.py). Never set in a timed run.
const char* even_stamps_path() {
    static const char* path = std::getenv("PSGD_EVEN_STAMPS");
    return path && *path ? path : nullptr;
}

int even_stamps_begin(psgd_plan* p, ProductArgs& pa) {
    if (!even_stamps_path()) return PSGD_OK;
    const size_t words = size_t(std::max(pa.nwg, 1)) * kEvenStamps;
    if (p->stamp_words < words) {
        if (p->stamp_buf) (void)hipFree(p->stamp_buf);
        p->stamp_buf = nullptr;
        PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&p->stamp_buf), words * sizeof(unsigned long long)));
        p->stamp_words = words;
    }
    PSGD_HIP(hipMemset(p->stamp_buf, 0, words * sizeof(unsigned long long)));
    pa.stamps = p->stamp_buf;
    return PSGD_OK;
}

int even_stamps_end(psgd_plan* p, const ProductArgs& pa, hipStream_t s) {
    if (!pa.stamps) return PSGD_OK;
    PSGD_HIP(hipStreamSynchronize(s));
    std::vector<unsigned long long> h(size_t(pa.nwg) * kEvenStamps);
    PSGD_HIP(hipMemcpy(h.data(), pa.stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    FILE* f = std::fopen(even_stamps_path(), "a");
    if (!f) return PSGD_OK;
    const int64_t esz = p->dtype == PSGD_BF16 ? 2 : 4;
    const int32_t w0 = int32_t((pa.wg_seg - p->dev(p->wg_seg)));
    std::fprintf(f, "%d", pa.nwg);
    for (int w = 0; w < pa.nwg; ++w) {
        int64_t bytes = 0;
        const int32_t b = p->wg_seg[size_t(w0 + w)], e = p->wg_seg[size_t(w0 + w + 1)];
        for (int32_t k = b; k < e; ++k) {
            const Seg& sg = p->segs[size_t(k)];
            const int64_t cols = std::min<int64_t>(int64_t(sg.lanes) * (sg.vec ? 4 : 1), sg.m - int64_t(sg.strip) * sg.lanes * (sg.vec ? 4 : 1));
            bytes += int64_t(sg.row1 - sg.row0) * cols * esz;
        }
        std::fprintf(f, " %d:%lld", e - b, static_cast<long long>(bytes));
        for (int k = 0; k < kEvenStamps; ++k) std::fprintf(f, ":%llu", h[size_t(w) * kEvenStamps + k]);
    }
    std::fprintf(f, "\n");
    std::fclose(f);
    return PSGD_OK;
}

}  // namespace

int psgd::compress_impl(psgd_plan* p, void* const* grads, int64_t step, int32_t it, hipStream_t s, StepCtx c) {
    if (p->f64()) return compress_f64(p, grads, step, it, s);
    if (p->wide()) return compress_wide(p, grads, step, it, s);
    if (int st = refresh_pointers(p, grads, s)) return st;
    const psgd_plan::Span sp = c.span ? *c.span : p->full_span();
    const bool even = p->even(step, it);
    float* in = even ? p->P : p->Q;
    float* out = even ? p->Q : p->P;
    const bool fused = p->fused_norm(c.fuse, it);
    // rank 1, iteration 0, even: the joint norm of the (raw) state P is folded into the even
    // product (per-chunk sums of squares) and its reduction (divide, write normalised P)
    const bool fused0 = p->rbucket == 1 && it == 0 && even && !p->fused_final_at(step, it, c.write_out);
    // projection form of the fused last iteration: its orthonormalisation leaves R' in o_rq
    const bool proj = it == p->iters - 1 && p->proj_final(step, c.write_out);
    // folded orthonormalisation of the projection form: the even reduction leaves Gram
    // partials and k_orth_chain (no Gram pass, panel rows over several workgroups) replaces
    // k_orth_chol
    const bool qf = p->qfold(step, c.write_out);
    const bool xg = c.xgram && it == 1 && !even;  // the exchange left the summed Q's Gram
    float* ss = p->dev<float>(p->o_ss);

    if ((qf && proj) || xg) {
        ChainArgs ca{};
        ca.units = p->dev(p->units_q) + sp.uq[0];
        ca.uitems = p->dev(p->uitems) + 2 * sp.uq[0];
        ca.gram = p->dev<double>(p->o_gram);
        // the even iteration's reduced Q: k_reduce's yloc (world size 1) or the exchange's
        // summed copy (history slot 2, psgd_aggregate_ipc)
        ca.raw = xg ? p->hist(2, it - 1) : p->hist(1, it - 1);
        ca.state = in;
        ca.hx = p->hist(0, it);
        ca.rfac = p->dev<float>(p->o_rq);
        PSGD_HIP(launch_orth_chain(ca, sp.uq[1] - sp.uq[0], p->panel_q, p->rbucket, s));
    } else if (!fused && !fused0) {
        OrthArgs oa{};
        const int32_t* ur = even ? sp.up : sp.uq;
        oa.units = p->dev(even ? p->units_p : p->units_q) + ur[0];
        oa.state = in;
        oa.hx = p->hist(0, it);
        oa.save = it > 0 ? p->hist(2, it - 1) : nullptr;  // keep the all-reduced factor of it-1
        oa.rfac = proj ? p->dev<float>(p->o_rq) : nullptr;
        const int nunits = ur[1] - ur[0];
        if (nunits > 0) PSGD_HIP(launch_orth(oa, nunits, p->rbucket, even ? p->panel_p : p->panel_q, p->orth_chol, s));
    }

    // where the previous iteration's reduction left the per-item sums of squares of its
    // out-factor (this iteration's raw in-factor) and the per-group item ranges (after an
    // odd-even pass the previous even reduction ran over its own item list)
    const float* prev_ss = ss + size_t((it - 1) & 1) * p->ss_stride;
    const bool oe_prev2 = !even && it >= 2 && p->oe_at(step, it - 2, c.write_out) && p->fused_norm(c.fuse, it - 2);
    const int32_t* prev_grng = p->dev(even ? p->grng_odd : oe_prev2 ? p->grng_oe_items : p->grng_even);
    // odd-even pass: this odd iteration and the next (even) one's product in one gradient pass
    // (k_final_oe); its P rows need no reduction, the even iteration reduces its partials
    if (fused && c.span == nullptr && p->oe_at(step, it, c.write_out)) {
        FinalArgs fa{};
        fa.mats = p->dev(p->mats);
        fa.tiles = p->dev(p->tiles_oe);
        const int nfin = int(p->tiles_oe.size());
        fa.grads = p->grad_tab.table();
        fa.x = p->hist(c.raw_slot, it - 1);
        fill_terms(p, step, it, fa.res);
        fa.nres = it;
        fa.yloc = p->hist(1, it);
        fa.state = out;
        fa.ss_in = prev_ss;
        fa.rng = p->dev(p->rng_oe);
        fa.rsel = oe_prev2 ? 1 : 0;  // (an odd iteration) the even items, or the ones after an odd-even pass
        fa.xstate = in;
        fa.hx = p->hist(0, it);
        fa.ntiles = nfin;
        fa.oe_part = p->dev<float>(p->o_oe_part);
        fa.oe_ss = p->dev<float>(p->o_oe_ss);
        PSGD_HIP(launch_final_oe(p->dtype, it, fin_bucket(p->fin_smax), fa, nfin, s, nullptr));
        return PSGD_OK;
    }
    const bool oe_prev = even && it >= 1 && c.span == nullptr && p->oe_at(step, it - 1, c.write_out) &&
                         p->fused_norm(c.fuse, it - 1);
    if (it == p->iters - 1 && p->fused_final(step, c.write_out)) {
        // last iteration, odd: product + residual (+ output at world size 1) in one pass
        FinalArgs fa{};
        fa.out_nt = p->out_nt;
        fa.mats = p->dev(p->mats);
        // the K-term form on its own row blocks when the plan has them (MatDesc::fin_rows_kt)
        const bool own_kt = !proj && !p->tiles_fin_kt.empty();
        const int32_t(&fr)[2] = own_kt ? sp.fin_kt : sp.fin;
        fa.tiles = p->dev(own_kt ? p->tiles_fin_kt : p->tiles_fin) + fr[0];
        fa.grads = p->grad_tab.table();
        fa.out = c.out;
        fa.x = fused ? p->hist(c.raw_slot, it - 1) : p->hist(0, it);
        fill_terms(p, step, it, fa.res);
        fa.nres = it;
        fa.write_out = c.write_out ? 1 : 0;
        fa.yloc = p->hist(1, it);
        fa.state = out;
        fa.xout = c.xout;
        if (fused) {
            fa.ss_in = prev_ss;  // the in-factor Q came from an even iteration's reduction
            fa.rng = p->dev(own_kt ? p->rng_fin_kt : p->rng_fin) + fr[0];
            fa.rsel = oe_prev2 ? 1 : 0;
            fa.xstate = in;
            fa.hx = p->hist(0, it);
        }
        const int nfin = fr[1] - fr[0];
        if (proj) {  // no error-feedback terms: P_0 and R' only (rank 1: P_0 and the matrix's c)
            fa.proj_p0 = p->hist(0, 0);
            fa.proj_r = p->dev<float>(p->o_rq);
            fill_terms(p, step, 0, fa.res);
            fa.nres = kFinProj;
        }
        fa.ntiles = nfin;
        if (c.fl && c.write_out) fa.flat = *c.fl;  // uncompressed tensors ride in the same launch
        if (nfin + fa.flat.nitems == 0) return PSGD_OK;
        std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
        if (int st = timing_begin(p, s, &ev, true)) return st;  // benchmark timing: the final pass
        TimedScope ts(ev);
        if (c.mix)  // psgd_aggregate_mixed: bf16 output, and the ingest fold of the single-pass form
            PSGD_HIP(launch_final_mix(p->rbucket, fa.nres, fin_bucket(p->fin_smax), c.mix_in && it == 0, fa, *c.mix, nfin,
                                      s, nullptr));
        else
            PSGD_HIP(launch_final_odd(p->dtype, p->rbucket, fa.nres, fin_bucket(p->fin_smax), fa, nfin, s));
        return PSGD_OK;
    }

    ProductArgs pa{};
    pa.mats = p->dev(p->mats);
    pa.grads = p->grad_tab.table();
    pa.x = fused ? p->hist(c.raw_slot, it - 1) : fused0 ? in : p->hist(0, it);  // fused: the raw factor
    pa.part = p->dev<float>(p->o_part);
    if (fused0) pa.ss0 = p->dev<float>(p->o_ss0);
    fill_terms(p, step, it, pa.res);
    pa.nres = it;
    if (oe_prev) {
        // the product of this even iteration was accumulated by the odd-even pass
    } else if (even) {
        // persistent k_even: this span's workgroups [wg[0], wg[1]) of the segmentation
        pa.segs = p->dev(p->segs);
        pa.wg_seg = p->dev(p->wg_seg) + sp.wg[0];
        pa.nwg = sp.wg[1] - sp.wg[0];
        // world size > 1 (no output written here): the first iteration's launch also packs the
        // uncompressed tensors, ahead of every collective
        if (c.fl && !c.write_out && it == 0) pa.flat = *c.fl;
        if (int st = even_stamps_begin(p, pa)) return st;
        PSGD_HIP(launch_even(p->dtype, p->rbucket, it, pa, pa.nwg, s));
        if (int st = even_stamps_end(p, pa, s)) return st;
    } else {
        if (sp.ov[1] > sp.ov[0]) {
            pa.tiles = p->dev(p->tiles_ov) + sp.ov[0];
            PSGD_HIP(launch_product_odd(p->dtype, p->rbucket, it, pa, sp.ov[1] - sp.ov[0], s));
        }
        if (sp.om[1] > sp.om[0]) {
            pa.tiles = p->dev(p->tiles_om) + sp.om[0];
            PSGD_HIP(launch_odd_mfma(p->dtype, p->rbucket, it, pa, sp.om[1] - sp.om[0], s));
        }
    }

    ReduceArgs ra{};
    ra.mats = pa.mats;
    const int32_t* rr = even ? sp.re : sp.ro;  // this parity's items (out-factor side)
    const int32_t* rn = even ? sp.ro : sp.re;  // the other parity's items (in-factor side)
    ra.items = p->dev(even ? p->red_even : p->red_odd) + rr[0];
    ra.part = pa.part;
    ra.yloc = p->hist(1, it);
    ra.state = out;
    ra.even = even ? 1 : 0;
    ra.nmain = rr[1] - rr[0];
    if (oe_prev) {  // the odd-even pass's block partials, per matrix [blocks][m]
        ra.items = p->dev(p->red_oe);
        ra.part = p->dev<float>(p->o_oe_part);
        ra.nmain = int32_t(p->red_oe.size());
    }
    if (fused0) {  // normalise the state P in place + history copy (P-side items)
        ra.ss_in = pa.ss0;
        ra.grng_in = p->dev(p->grng_ss0);
        ra.nitems = p->dev(p->red_odd) + sp.ro[0];
        ra.nnorm = sp.ro[1] - sp.ro[0];
        ra.raw = in;
        ra.xstate = in;
        ra.hx = p->hist(0, it);
    }
    if (fused) {  // in-factor items: the other parity's item list (in-factor side)
        ra.ss_in = oe_prev ? p->dev<float>(p->o_oe_ss) : prev_ss;  // odd-even: the blocks' sums of P^2
        ra.grng_in = oe_prev ? p->dev(p->grng_oe) : prev_grng;
        ra.nitems = p->dev(even ? p->red_odd : p->red_even) + rn[0];
        ra.nnorm = rn[1] - rn[0];
        ra.raw = p->hist(c.raw_slot, it - 1);
        ra.xstate = in;
        ra.hx = p->hist(0, it);
    }
    // ss_out is indexed by the launch's block (item) index: offset like the item list
    if (p->fused_norm(c.fuse, it + 1) && it + 1 < p->iters) ra.ss_out = ss + size_t(it & 1) * p->ss_stride + rr[0];
    ra.xout = c.xout;
    if (qf && even && it + 2 == p->iters) {  // the Q panels' Gram for k_orth_chain
        ra.gram = p->dev<double>(p->o_gram) + size_t(rr[0]) * kGramStride;
        ra.gram_r = p->rbucket;
    }
    if (ra.nmain + ra.nnorm > 0) PSGD_HIP(launch_reduce(ra, ra.nmain + ra.nnorm, s));
    return PSGD_OK;
}

int psgd::aggregate_ctx(psgd_plan* p, void* const* grads, int64_t step, hipStream_t s, StepCtx c) {
    c.fuse = c.write_out = true;
    for (int it = 0; it < p->iters; ++it)
        if (int st = compress_impl(p, grads, step, it, s, c)) return st;
    if (p->fused_final(step, true)) return PSGD_OK;  // output written by the fused last iteration
    return decompress_impl(p, grads, c.out, step, 1, s, c);
}

int psgd::decompress_impl(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world, hipStream_t s,
                          StepCtx c) {
    if (p->f64()) return decompress_f64(p, grads, out, step, world, s);
    if (p->wide()) return decompress_wide(p, grads, out, step, world, s);
    if (int st = refresh_pointers(p, grads, s)) return st;
    const psgd_plan::Span sp = c.span ? *c.span : p->full_span();
    const int nt = sp.tiles[1] - sp.tiles[0];
    const int I = p->iters;
    ApplyArgs aa{};
    aa.mats = p->dev(p->mats);
    aa.tiles = p->dev(p->tiles) + sp.tiles[0];
    aa.grads = p->grad_tab.table();
    aa.out = out;
    fill_terms(p, step, I, aa.res);
    float* last = p->even(step, I - 1) ? p->Q : p->P;  // all-reduced factor of the last iteration
    for (int k = 0; k < kMaxTerms; ++k) aa.apx.p[k] = aa.apx.q[k] = nullptr;
    for (int k = 0; k < I; ++k) {
        const bool e = p->even(step, k);
        // fused (world 1): the reduced factor was never copied to hist(2): use hist(1)
        float* ybar = k + 1 < I ? p->hist(p->fused_norm(c.fuse, k + 1) ? 1 : 2, k) : last;
        aa.apx.p[k] = e ? p->hist(0, k) : ybar;
        aa.apx.q[k] = e ? ybar : p->hist(0, k);
    }
    aa.nterms = I;
    aa.alpha = float(1.0 / double(world));  // reference alpha = 1 / num_workers (:218)
    aa.out_nt = world == 1 ? p->out_nt : 0;
    if (p->fused_final(step, false)) {
        // the residual was written by the fused last iteration: output only
        aa.ntiles = nt;
        if (c.mix) {  // psgd_aggregate_mixed_comm: bf16 output, the flat tail's round items first
            if (c.fl) aa.flat = *c.fl;
            if (nt + aa.flat.nitems > 0) PSGD_HIP(launch_lowrank_mix(p->rbucket, I, aa, *c.mix, nt, s, nullptr));
            return PSGD_OK;
        }
        if (nt > 0) PSGD_HIP(launch_lowrank_out(p->dtype, p->rbucket, I, aa, nt, s));
        return PSGD_OK;
    }
    aa.ntiles = nt;
    if (c.fl) aa.flat = *c.fl;  // uncompressed tensors ride in the same launch
    if (nt + aa.flat.nitems == 0) return PSGD_OK;
    std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
    if (int st = timing_begin(p, s, &ev, true)) return st;
    TimedScope ts(ev);
    if (c.mix && world == 1)  // psgd_aggregate_mixed (world size 1): bf16 output
        PSGD_HIP(launch_apply_mix(p->rbucket, I, aa, *c.mix, nt, s, nullptr));
    else if (c.mix)  // psgd_aggregate_mixed_comm at W > 1: two term sets, bf16 output
        PSGD_HIP(launch_apply_mix_w(p->rbucket, I, aa, *c.mix, nt, s, nullptr));
    else
        PSGD_HIP(launch_apply(p->dtype, p->rbucket, I, world == 1, aa, nt, s));
    return PSGD_OK;
}

namespace {

int bucket_span(const psgd_plan* p, int32_t b, psgd_plan::Span* sp) {
    if (p->f64()) return fail(PSGD_ERR_DTYPE, "buckets are not supported for fp64 plans");
    if (int st = refuse_wide(p, "psgd_compress_bucket / psgd_decompress_bucket")) return st;
    if (p->spans.empty()) {
        if (b != 0) return fail(PSGD_ERR_VALUE, "bucket out of range");
        *sp = p->full_span();
        return PSGD_OK;
    }
    if (b < 0 || b >= int32_t(p->spans.size())) return fail(PSGD_ERR_VALUE, "bucket out of range");
    *sp = p->spans[b];
    return PSGD_OK;
}

// World-size-1 step (psgd_aggregate / psgd_aggregate_flat): the rank-1 joint norm folded, the
// output written by the fused last iteration where the plan has one
int aggregate_impl(psgd_plan* p, void* const* grads, void* out, int64_t step, hipStream_t s, const FlatArgs* fl) {
    StepCtx c;
    c.fl = fl;
    c.out = out;
    return aggregate_ctx(p, grads, step, s, c);
}

int check_terms(int32_t nterms, const float* const* a, const float* const* b) {
    if (nterms < 0 || nterms > kMaxTerms) return fail(PSGD_ERR_VALUE, "term count out of range");
    for (int k = 0; k < nterms; ++k)
        if (!a || !b || !a[k] || !b[k]) return fail(PSGD_ERR_VALUE, "null term buffer");
    return PSGD_OK;
}

// select (or upload, stream-ordered) a per-tensor destination table; every pointer must keep
// the vector layout's alignment where the matrix uses it
int refresh_table(psgd_plan* p, void* const* ptrs, TableCache& tab, hipStream_t s) {
    const uintptr_t need = p->dtype == PSGD_F32 ? 16 : 8;
    for (const MatDesc& md : p->mats) {
        if (!ptrs[md.tensor]) return fail(PSGD_ERR_VALUE, "null destination pointer");
        if (md.vec && reinterpret_cast<uintptr_t>(ptrs[md.tensor]) % need)
            return fail(PSGD_ERR_LAYOUT, "destination tensor is not aligned for the vector layout");
    }
    PSGD_HIP(tab.select(ptrs, s));
    return PSGD_OK;
}

}  // namespace

// `mix` (psgd_aggregate_mixed_comm): `grads` the fp32 residual, `out` / `flat_out` bf16, `unc` the
// uncompressed tensors' fp32 residual; the flat tail is staged in mix->stage (fp32) around its
// collective: ingest-pack in a launch of its own first, the round items in the final launch
int psgd::aggregate_comm_ctx(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f,
                             void* const* unc, void* flat_out, psgd_comm* comm, hipStream_t s, const MixArgs* mix) {
    const bool has_flat = f != nullptr;
    const int world = comm_world(comm);
    // x / W into the flat buffer, x = 0 (utils.py:43-47, powersgd.py:29-30): inside the first
    // even product's launch when the step starts even, else its own launch
    FlatArgs fa{};
    const bool fold = has_flat && !mix && p->even(step, 0) && !p->wide();  // wide products carry no flat pack
    if (fold || (mix && has_flat)) {
        if (int st = flat_args(f, unc, flat_out, world, s, &fa)) return st;
        if (mix) PSGD_HIP(launch_flat_ingest(fa, *mix, s));
    } else if (has_flat) {
        if (int st = psgd_flat_pack(f, unc, flat_out, world, s)) return st;
    }
    float* const tail = mix ? mix->stage : static_cast<float*>(flat_out);
    StepCtx c;
    c.fl = fold ? &fa : nullptr;
    for (int it = 0; it < p->iters; ++it) {
        if (int st = compress_impl(p, grads, step, it, s, c)) return st;
        const bool e = p->even(step, it);
        const bool last = it == p->iters - 1;
        if (int st = comm_allreduce(comm, e ? p->Q : p->P, size_t(e ? p->qtot : p->ptot),
                                    last && has_flat ? tail : nullptr, last && has_flat ? size_t(f->total) : 0, s))
            return st;
    }
    if (!mix) return decompress_impl(p, grads, out, step, world, s, StepCtx{});
    // the round items ride in every final launch built for them; a 1-rank communicator's unfused
    // final pass is the world-size-1 instance, whose flat items ingest: the round follows it
    const bool ride = world > 1 || p->fused_final(step, false);
    StepCtx d;
    d.mix = mix;
    d.fl = has_flat && ride ? &fa : nullptr;
    if (int st = decompress_impl(p, grads, out, step, world, s, d)) return st;
    if (has_flat && !ride) PSGD_HIP(launch_flat_round(fa, *mix, s));
    return PSGD_OK;
}

namespace {

int aggregate_comm_body(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f,
                        void* const* unc, void* flat_out, psgd_comm* comm, hipStream_t s) {
    return aggregate_comm_ctx(p, grads, out, step, f, unc, flat_out, comm, s, nullptr);
}

}  // namespace

extern "C" {

int psgd_compress(psgd_plan* p, void* const* grads, int64_t step, int32_t it, void* stream) {
    if (!p || !grads) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (step < 0 || it < 0 || it >= p->iters) return fail(PSGD_ERR_VALUE, "step/iteration out of range");
    DevScope scope(p->device);
    return compress_impl(p, grads, step, it, static_cast<hipStream_t>(stream), StepCtx{});
}

int psgd_decompress(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world,
                    void* stream) {
    if (!p || !grads || !out) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (step < 0 || world < 1) return fail(PSGD_ERR_VALUE, "step/world size out of range");
    if (reinterpret_cast<uintptr_t>(out) % 16) return fail(PSGD_ERR_LAYOUT, "output buffer must be 16-byte aligned");
    DevScope scope(p->device);
    return decompress_impl(p, grads, out, step, world, static_cast<hipStream_t>(stream), StepCtx{});
}

int psgd_compress_bucket(psgd_plan* p, void* const* grads, int64_t step, int32_t it, int32_t bucket, void* stream) {
    if (!p || !grads) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (step < 0 || it < 0 || it >= p->iters) return fail(PSGD_ERR_VALUE, "step/iteration out of range");
    psgd_plan::Span sp;
    if (int st = bucket_span(p, bucket, &sp)) return st;
    DevScope scope(p->device);
    StepCtx c;
    c.span = &sp;
    return compress_impl(p, grads, step, it, static_cast<hipStream_t>(stream), c);
}

int psgd_decompress_bucket(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world, int32_t bucket,
                           void* stream) {
    if (!p || !grads || !out) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (step < 0 || world < 1) return fail(PSGD_ERR_VALUE, "step/world size out of range");
    if (reinterpret_cast<uintptr_t>(out) % 16) return fail(PSGD_ERR_LAYOUT, "output buffer must be 16-byte aligned");
    psgd_plan::Span sp;
    if (int st = bucket_span(p, bucket, &sp)) return st;
    DevScope scope(p->device);
    StepCtx c;
    c.span = &sp;
    return decompress_impl(p, grads, out, step, world, static_cast<hipStream_t>(stream), c);
}

// World size 1: the pointer tables are selected (or uploaded) on the caller's stream, then the
// step's launches follow on it.
int psgd_aggregate(psgd_plan* p, void* const* grads, void* out, int64_t step, void* stream) {
    if (!p || !grads || !out) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (reinterpret_cast<uintptr_t>(out) % 16) return fail(PSGD_ERR_LAYOUT, "output buffer must be 16-byte aligned");
    DevScope scope(p->device);
    return aggregate_impl(p, grads, out, step, static_cast<hipStream_t>(stream), nullptr);
}

int psgd_aggregate_flat(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f,
                        void* const* unc, void* flat_out, void* stream) {
    if (!f || f->total == 0) return psgd_aggregate(p, grads, out, step, stream);
    if (!p || !grads || !out || !unc || !flat_out) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound || !f->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (reinterpret_cast<uintptr_t>(out) % 16) return fail(PSGD_ERR_LAYOUT, "output buffer must be 16-byte aligned");
    if (f->dtype != p->dtype || f->device != p->device || p->f64() || p->wide()) {  // separate launches
        if (int st = psgd_aggregate(p, grads, out, step, stream)) return st;
        return psgd_flat_pack(f, unc, flat_out, 1, stream);
    }
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FlatArgs a;
    if (int st = flat_args(f, unc, flat_out, 1, s, &a)) return st;
    return aggregate_impl(p, grads, out, step, s, &a);
}

// World size W in one call (include/psgd.h): per iteration the kernels, then the in-place SUM
// all-reduce of the out-factor state on the same stream (the last grouped with the flat
// buffer of the uncompressed tensors), then the output pass. Same sequence as the building
// blocks psgd_compress / all_reduce / psgd_decompress (reference powersgd.py:172-230).
int psgd_aggregate_comm(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f, void* const* unc,
                        void* flat_out, psgd_comm* comm, void* stream) {
    if (!p || !grads || !out || !comm) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (p->f64()) return fail(PSGD_ERR_DTYPE, "psgd_aggregate_comm takes fp32/bf16 plans (fp32 factors)");
    if (reinterpret_cast<uintptr_t>(out) % 16) return fail(PSGD_ERR_LAYOUT, "output buffer must be 16-byte aligned");
    const bool has_flat = f && f->total > 0;
    if (has_flat) {
        if (!unc || !flat_out) return fail(PSGD_ERR_VALUE, "null argument");
        if (!f->bound) return fail(PSGD_ERR_STATE, "flat plan is not bound");
        if (f->dtype != PSGD_F32) return fail(PSGD_ERR_DTYPE, "psgd_aggregate_comm packs fp32 uncompressed tensors");
    }
    // a poisoned communicator is refused before the step launches anything: the caller's
    // gradients and the P/Q state stay as they were
    std::string why;
    if (comm_poisoned(comm, &why))
        return fail(PSGD_ERR_STATE, ("communicator unusable after an earlier failure: " + why).c_str());
    DevScope scope(p->device);
    const int st = aggregate_comm_body(p, grads, out, step, has_flat ? f : nullptr, unc, flat_out, comm,
                                       static_cast<hipStream_t>(stream));
    // a failure past the argument checks can leave this rank's collective sequence short of its
    // peers': the communicator refuses every later call (psgd_comm.cpp, comm_poison)
    if (st) comm_poison(comm, psgd_last_error());
    return st;
}

// ------------------------------------------------- building blocks (reducer variants) ---
int psgd_product(psgd_plan* p, void* const* grads, int32_t odd, const float* x, float* y, int32_t nterms,
                 const float* const* term_p, const float* const* term_q, void* stream) {
    if (!p || !grads || !x || !y) return fail(PSGD_ERR_VALUE, "null argument");
    if (p->f64()) return fail(PSGD_ERR_DTYPE, "the building blocks take fp32/bf16 plans");
    if (int st = refuse_wide(p, "psgd_product")) return st;
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (int st = check_terms(nterms, term_p, term_q)) return st;
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int st = refresh_pointers(p, grads, s)) return st;
    ProductArgs pa{};
    pa.mats = p->dev(p->mats);
    pa.grads = p->grad_tab.table();
    pa.x = x;
    pa.part = p->dev<float>(p->o_part);
    for (int k = 0; k < nterms; ++k) {
        pa.res.p[k] = term_p[k];
        pa.res.q[k] = term_q[k];
    }
    pa.nres = nterms;
    if (!odd) {
        pa.segs = p->dev(p->segs);
        pa.wg_seg = p->dev(p->wg_seg);
        pa.nwg = int(p->wg_seg.size()) - 1;
        PSGD_HIP(launch_even(p->dtype, p->rbucket, nterms, pa, pa.nwg, s));
    } else {
        if (!p->tiles_ov.empty()) {
            pa.tiles = p->dev(p->tiles_ov);
            PSGD_HIP(launch_product_odd(p->dtype, p->rbucket, nterms, pa, int(p->tiles_ov.size()), s));
        }
        if (!p->tiles_om.empty()) {
            pa.tiles = p->dev(p->tiles_om);
            PSGD_HIP(launch_odd_mfma(p->dtype, p->rbucket, nterms, pa, int(p->tiles_om.size()), s));
        }
    }
    ReduceArgs ra{};
    ra.mats = pa.mats;
    ra.items = p->dev(odd ? p->red_odd : p->red_even);
    ra.part = pa.part;
    ra.yloc = y;
    ra.state = y;
    ra.even = odd ? 0 : 1;
    ra.nmain = int(odd ? p->red_odd.size() : p->red_even.size());
    PSGD_HIP(launch_reduce(ra, ra.nmain, s));
    return PSGD_OK;
}

int psgd_orthogonalize(psgd_plan* p, int32_t which, float* buf, int32_t mode, void* stream) {
    if (!p || !buf) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (mode != 0 && mode != 1) return fail(PSGD_ERR_VALUE, "mode must be 0 (reference) or 1 (paper-code)");
    if (p->f64()) return fail(PSGD_ERR_DTYPE, "the building blocks take fp32/bf16 plans");
    if (int st = refuse_wide(p, "psgd_orthogonalize")) return st;
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    OrthArgs oa{};
    oa.state = buf;
    oa.hx = p->hist(0, 0);  // scratch copy
    if (mode == 1) {
        oa.units = p->dev(which ? p->munits_p : p->munits_q);
        PSGD_HIP(launch_orth_mgs(oa, int(p->mats.size()), p->rbucket, s));
    } else {
        oa.units = p->dev(which ? p->units_p : p->units_q);
        const int nunits = int(which ? p->units_p.size() : p->units_q.size());
        PSGD_HIP(launch_orth(oa, nunits, p->rbucket, which ? p->panel_p : p->panel_q, p->orth_chol, s));
    }
    return PSGD_OK;
}

int psgd_reconstruct(psgd_plan* p, void* const* grads, void* const* resid_out, void* const* out, int32_t nterms,
                     const float* const* term_p, const float* const* term_q, const float* const* avg_p,
                     const float* const* avg_q, float alpha, void* stream) {
    if (!p || !grads || !out) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (nterms < 1) return fail(PSGD_ERR_VALUE, "at least one term");
    if (p->f64()) return fail(PSGD_ERR_DTYPE, "the building blocks take fp32/bf16 plans");
    if (int st = refuse_wide(p, "psgd_reconstruct")) return st;
    if (int st = check_terms(nterms, term_p, term_q)) return st;
    if (int st = check_terms(nterms, avg_p, avg_q)) return st;
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int st = refresh_pointers(p, grads, s)) return st;
    if (resid_out)
        if (int st = refresh_table(p, resid_out, p->rdst_tab, s)) return st;
    if (int st = refresh_table(p, out, p->odst_tab, s)) return st;
    ApplyArgs aa{};
    aa.mats = p->dev(p->mats);
    aa.tiles = p->dev(p->tiles);
    aa.grads = p->grad_tab.table();
    aa.rdst = resid_out ? p->rdst_tab.table() : nullptr;
    aa.odst = p->odst_tab.table();
    bool shared = alpha == 1.0f;
    for (int k = 0; k < nterms; ++k) {
        aa.res.p[k] = term_p[k];
        aa.res.q[k] = term_q[k];
        aa.apx.p[k] = avg_p[k];
        aa.apx.q[k] = avg_q[k];
        shared = shared && avg_p[k] == term_p[k] && avg_q[k] == term_q[k];
    }
    aa.nterms = nterms;
    aa.alpha = alpha;
    aa.ntiles = int32_t(p->tiles.size());
    PSGD_HIP(launch_apply(p->dtype, p->rbucket, nterms, shared, aa, int(p->tiles.size()), s));
    return PSGD_OK;
}

}  // extern "C"
