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

// The first `count` rank-r terms of a step from the factor history: iteration j's in-factor x(j)
// and out-factor y(j); even -> (P_j = X_j, Q_j = Y_j), odd -> (P_j = Y_j, Q_j = X_j). The output
// terms of the three decompress drivers take the all-reduced out-factor for y
template <typename TermsT, typename X, typename Y>
void fill_terms(const psgd_plan* p, int64_t step, int count, TermsT& res, X x, Y y) {
    for (int j = 0; j < count; ++j) {
        const bool e = p->even(step, j);
        res.p[j] = e ? x(j) : y(j);
        res.q[j] = e ? y(j) : x(j);
    }
    for (int j = count; j < kMaxTerms; ++j) res.p[j] = res.q[j] = nullptr;
}
// the local terms (error feedback): history slots 0 and 1
void fill_terms(const psgd_plan* p, int64_t step, int count, Terms& res) {
    fill_terms(p, step, count, res, [p](int j) { return p->hist(0, j); }, [p](int j) { return p->hist(1, j); });
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
    fill_terms(p, step, count, res, [p](int j) { return p->hist64(0, j); }, [p](int j) { return p->hist64(1, j); });
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
    fill_terms(p, step, I, a.apx, [&](int k) { return p->hist64(0, k); },
               [&](int k) { return k + 1 < I ? p->hist64(2, k) : last; });  // all-reduced factor of iteration k
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
// `xout` (psgd_aggregate_ipc): the reduction also writes the local out-factor into this rank's
// exchange slot.
int compress_wide(psgd_plan* p, void* const* grads, int64_t step, int32_t it, hipStream_t s, float* xout) {
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
    a.xout = xout;
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
    fill_terms(p, step, I, a.apx, [&](int k) { return p->hist(0, k); },
               [&](int k) { return k + 1 < I ? p->hist(2, k) : last; });
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

namespace {

// ------------------------------------------------- fp32 / bf16 plans up to rank 32 ------
// One helper per stage of an iteration; each fills one argument struct from the route
// (psgd_plan.h, IterRoute) and launches. None of them re-derives a flag.
struct Iter {
    psgd_plan* p;
    int64_t step;
    int it;
    IterRoute r;
    psgd_plan::Span sp;
    hipStream_t s;
    const StepCtx& c;
    float* in() const { return r.even ? p->P : p->Q; }
    float* out() const { return r.even ? p->Q : p->P; }
    // where the previous iteration's reduction left the per-item sums of squares of its
    // out-factor (this iteration's raw in-factor)
    const float* prev_ss() const { return p->dev<float>(p->o_ss) + size_t((it - 1) & 1) * p->ss_stride; }
};

int orth_stage(const Iter& i) {
    psgd_plan* p = i.p;
    if (i.r.orth == IterRoute::OrthChain) {
        ChainArgs ca{};
        ca.units = p->dev(p->units_q) + i.sp.uq[0];
        ca.uitems = p->dev(p->uitems) + 2 * i.sp.uq[0];
        ca.gram = p->dev<double>(p->o_gram);
        // the even iteration's reduced Q: k_reduce's yloc (world size 1) or the exchange's
        // summed copy (history slot 2, psgd_aggregate_ipc)
        ca.raw = p->hist(i.r.chain_from_exchange ? 2 : 1, i.it - 1);
        ca.state = i.in();
        ca.hx = p->hist(0, i.it);
        ca.rfac = p->dev<float>(p->o_rq);
        PSGD_HIP(launch_orth_chain(ca, i.sp.uq[1] - i.sp.uq[0], p->panel_q, p->rbucket, i.s));
    } else if (i.r.orth == IterRoute::OrthLaunch) {
        OrthArgs oa{};
        const int32_t* ur = i.r.even ? i.sp.up : i.sp.uq;
        oa.units = p->dev(i.r.even ? p->units_p : p->units_q) + ur[0];
        oa.state = i.in();
        oa.hx = p->hist(0, i.it);
        oa.save = i.it > 0 ? p->hist(2, i.it - 1) : nullptr;  // keep the all-reduced factor of it-1
        oa.rfac = i.r.proj ? p->dev<float>(p->o_rq) : nullptr;
        const int nunits = ur[1] - ur[0];
        if (nunits > 0)
            PSGD_HIP(launch_orth(oa, nunits, p->rbucket, i.r.even ? p->panel_p : p->panel_q, p->orth_chol, i.s));
    }
    return PSGD_OK;
}

// what k_final_oe and the fused last iteration share: the in-factor (raw, with the previous
// reduction's sums of squares, when the rank-1 norm is folded), the earlier terms, the out-factor
FinalArgs final_args(const Iter& i) {
    const psgd_plan* p = i.p;
    FinalArgs fa{};
    fa.mats = p->dev(p->mats);
    fa.grads = p->grad_tab.table();
    fa.x = i.r.fused ? p->hist(i.c.raw_slot, i.it - 1) : p->hist(0, i.it);
    fill_terms(p, i.step, i.it, fa.res);
    fa.nres = i.it;
    fa.yloc = p->hist(1, i.it);
    fa.state = i.out();
    if (i.r.fused) {
        fa.ss_in = i.prev_ss();  // the in-factor Q came from an even iteration's reduction
        fa.rsel = i.r.prev_after_oe ? 1 : 0;  // the even items, or the ones after an odd-even pass
        fa.xstate = i.in();
        fa.hx = p->hist(0, i.it);
    }
    return fa;
}

// odd-even pass: this odd iteration and the next (even) one's product in one gradient pass
// (k_final_oe); its P rows need no reduction, the even iteration reduces its partials
int odd_even_stage(const Iter& i) {
    const psgd_plan* p = i.p;
    FinalArgs fa = final_args(i);
    fa.tiles = p->dev(p->tiles_oe);
    fa.rng = p->dev(p->rng_oe);
    fa.ntiles = int32_t(p->tiles_oe.size());
    fa.oe_part = p->dev<float>(p->o_oe_part);
    fa.oe_ss = p->dev<float>(p->o_oe_ss);
    PSGD_HIP(launch_final_oe(p->dtype, i.it, fin_bucket(p->fin_smax), fa, fa.ntiles, i.s, nullptr));
    return PSGD_OK;
}

// last iteration, odd: product + residual (+ output at world size 1) in one pass
int final_stage(const Iter& i) {
    psgd_plan* p = i.p;
    const StepCtx& c = i.c;
    FinalArgs fa = final_args(i);
    fa.out_nt = p->out_nt;
    // the K-term form on its own row blocks when the plan has them (MatDesc::fin_rows_kt)
    const int32_t(&fr)[2] = i.r.own_kt ? i.sp.fin_kt : i.sp.fin;
    fa.tiles = p->dev(i.r.own_kt ? p->tiles_fin_kt : p->tiles_fin) + fr[0];
    if (i.r.fused) fa.rng = p->dev(i.r.own_kt ? p->rng_fin_kt : p->rng_fin) + fr[0];
    fa.out = c.out;
    fa.write_out = c.write_out ? 1 : 0;
    fa.xout = c.xout;
    if (i.r.proj) {  // no error-feedback terms: P_0 and R' only (rank 1: P_0 and the matrix's c)
        fa.proj_p0 = p->hist(0, 0);
        fa.proj_r = p->dev<float>(p->o_rq);
        fill_terms(p, i.step, 0, fa.res);
    }
    fa.nres = i.r.final_nres;
    fa.ntiles = fr[1] - fr[0];
    if (c.fl && c.write_out) fa.flat = *c.fl;  // uncompressed tensors ride in the same launch
    if (fa.ntiles + fa.flat.nitems == 0) return PSGD_OK;
    if (c.write_out && c.span == nullptr) {
        // this pass writes the output (world size 1): the terms psgd_clip_outputs reads afterwards
        // are the local ones, history slots 0 / 1 and this iteration's P in the state buffer (the
        // projection form's output G0 X X^T is P0 Q0^T + P1 X^T with P1 = G0 X - P0 R'^T, the state)
        Terms apx;
        fill_terms(p, i.step, p->iters, apx, [p](int k) { return p->hist(0, k); },
                   [&](int k) { return k + 1 < p->iters ? p->hist(1, k) : i.out(); });
        p->record_terms(i.step, 1, apx, p->iters, 1.f);
    }
    std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
    if (int st = timing_begin(p, i.s, &ev, true)) return st;  // benchmark timing: the final pass
    TimedScope ts(ev);
    PSGD_HIP(launch_final_pass(p, i.r, fa, c.mix, fa.ntiles, i.s, nullptr));
    return PSGD_OK;
}

// the fixed-order reduction of the product's partials into the out-factor; with the rank-1 norm
// folded it also normalises the in-factor (its items follow the main ones)
int reduce_stage(const Iter& i, const ProductArgs& pa) {
    psgd_plan* p = i.p;
    const StepCtx& c = i.c;
    const IterRoute& r = i.r;
    const psgd_plan::Span& sp = i.sp;
    const bool from_oe = r.pass == IterRoute::PassFromOddEven;
    ReduceArgs ra{};
    ra.mats = pa.mats;
    const int32_t* rr = r.even ? sp.re : sp.ro;  // this parity's items (out-factor side)
    const int32_t* rn = r.even ? sp.ro : sp.re;  // the other parity's items (in-factor side)
    ra.items = p->dev(r.even ? p->red_even : p->red_odd) + rr[0];
    ra.part = pa.part;
    ra.yloc = p->hist(1, i.it);
    ra.state = i.out();
    ra.even = r.even ? 1 : 0;
    ra.nmain = rr[1] - rr[0];
    if (from_oe) {  // the odd-even pass's block partials, per matrix [blocks][m]
        ra.items = p->dev(p->red_oe);
        ra.part = p->dev<float>(p->o_oe_part);
        ra.nmain = int32_t(p->red_oe.size());
    }
    if (r.fused0) {  // normalise the state P in place + history copy (P-side items)
        ra.ss_in = pa.ss0;
        ra.grng_in = p->dev(p->grng_ss0);
        ra.nitems = p->dev(p->red_odd) + sp.ro[0];
        ra.nnorm = sp.ro[1] - sp.ro[0];
        ra.raw = i.in();
    }
    if (r.fused) {  // in-factor items: the other parity's item list; after an odd-even pass the
                    // blocks' sums of P^2, and the previous even reduction ran over red_oe
        ra.ss_in = from_oe ? p->dev<float>(p->o_oe_ss) : i.prev_ss();
        ra.grng_in = p->dev(from_oe ? p->grng_oe : r.even ? p->grng_odd : r.prev_after_oe ? p->grng_oe_items : p->grng_even);
        ra.nitems = p->dev(r.even ? p->red_odd : p->red_even) + rn[0];
        ra.nnorm = rn[1] - rn[0];
        ra.raw = p->hist(c.raw_slot, i.it - 1);
    }
    if (r.fused || r.fused0) {
        ra.xstate = i.in();
        ra.hx = p->hist(0, i.it);
    }
    // ss_out is indexed by the launch's block (item) index: offset like the item list
    if (r.ss_out) ra.ss_out = p->dev<float>(p->o_ss) + size_t(i.it & 1) * p->ss_stride + rr[0];
    ra.xout = c.xout;
    if (r.gram_out) {  // the Q panels' Gram for k_orth_chain
        ra.gram = p->dev<double>(p->o_gram) + size_t(rr[0]) * kGramStride;
        ra.gram_r = p->rbucket;
    }
    if (ra.nmain + ra.nnorm > 0) PSGD_HIP(launch_reduce(ra, ra.nmain + ra.nnorm, i.s));
    return PSGD_OK;
}


// the product of PassEven / PassOdd (PassFromOddEven: accumulated by the odd-even pass, no
// launch), then its reduction
int product_stage(const Iter& i) {
    psgd_plan* p = i.p;
    const StepCtx& c = i.c;
    const IterRoute& r = i.r;
    const psgd_plan::Span& sp = i.sp;
    ProductArgs pa{};
    pa.mats = p->dev(p->mats);
    pa.grads = p->grad_tab.table();
    pa.x = r.fused ? p->hist(c.raw_slot, i.it - 1) : r.fused0 ? i.in() : p->hist(0, i.it);  // fused: the raw factor
    pa.part = p->dev<float>(p->o_part);
    if (r.fused0) pa.ss0 = p->dev<float>(p->o_ss0);
    fill_terms(p, i.step, i.it, pa.res);
    pa.nres = i.it;
    if (r.pass == IterRoute::PassEven) {
        // persistent k_even: this span's workgroups [wg[0], wg[1]) of the segmentation
        pa.segs = p->dev(p->segs);
        pa.wg_seg = p->dev(p->wg_seg) + sp.wg[0];
        pa.nwg = sp.wg[1] - sp.wg[0];
        // world size > 1 (no output written here): the first iteration's launch also packs the
        // uncompressed tensors, ahead of every collective
        if (c.fl && !c.write_out && i.it == 0) pa.flat = *c.fl;
        if (int st = even_stamps_begin(p, pa)) return st;
        PSGD_HIP(launch_even(p->dtype, p->rbucket, i.it, pa, pa.nwg, i.s));
        if (int st = even_stamps_end(p, pa, i.s)) return st;
    } else if (r.pass == IterRoute::PassOdd) {
        if (sp.ov[1] > sp.ov[0]) {
            pa.tiles = p->dev(p->tiles_ov) + sp.ov[0];
            PSGD_HIP(launch_product_odd(p->dtype, p->rbucket, i.it, pa, sp.ov[1] - sp.ov[0], i.s));
        }
        if (sp.om[1] > sp.om[0]) {
            pa.tiles = p->dev(p->tiles_om) + sp.om[0];
            PSGD_HIP(launch_odd_mfma(p->dtype, p->rbucket, i.it, pa, sp.om[1] - sp.om[0], i.s));
        }
    }
    return reduce_stage(i, pa);
}
}  // namespace

hipError_t psgd::launch_final_pass(const psgd_plan* p, const IterRoute& r, const FinalArgs& a, const MixArgs* mix,
                                   int ntiles, hipStream_t s, int* waves) {
    const int smax = fin_bucket(p->fin_smax);
    if (smax == 0) return hipErrorInvalidValue;  // no instance serves rows of that many segments
    if (mix)  // psgd_aggregate_mixed: bf16 output, and the ingest fold of the single-pass form
        return launch_final_mix(p->rbucket, r.final_nres, smax, r.ingest, a, *mix, ntiles, s, waves);
    return launch_final_odd(p->dtype, p->rbucket, r.final_nres, smax, a, ntiles, s, waves);
}

hipError_t psgd::launch_out_pass(const psgd_plan* p, const OutRoute& o, ApplyArgs& a, const MixArgs* mix, int ntiles,
                                 hipStream_t s, int* waves, const MixDst* dst, const DirectDst* fdst) {
    a.out_nt = o.out_nt;
    const int R = p->rbucket, I = p->iters;
    if (o.fdst) {  // psgd_aggregate_comm_dst: the fp32 averages go to the per-tensor destinations
        if (p->dtype != PSGD_F32) return hipErrorInvalidValue;
        a.odst = fdst->dst;
        if (o.kind == OutRoute::Lowrank) return launch_lowrank_dst(R, I, a, *fdst, ntiles, s, waves);
        return launch_apply_dst(R, I, o.shared, a, *fdst, ntiles, s, waves);
    }
    if (o.dst) {  // psgd_aggregate_mixed_comm_dst: the averages go to the per-tensor destinations
        a.odst = dst->dst;
        if (o.kind == OutRoute::Lowrank) return launch_lowrank_mix_dst(R, I, a, *mix, dst->unc_dst, ntiles, s, waves);
        if (o.inst == OutRoute::MixW) return launch_apply_mix_w_dst(R, I, a, *mix, dst->unc_dst, ntiles, s, waves);
        return launch_apply_mix_dst(R, I, a, ntiles, s, waves);
    }
    if (o.kind == OutRoute::Lowrank)
        return mix ? launch_lowrank_mix(R, I, a, *mix, ntiles, s, waves) : launch_lowrank_out(p->dtype, R, I, a, ntiles, s);
    switch (o.inst) {
        case OutRoute::Mix: return launch_apply_mix(R, I, a, *mix, ntiles, s, waves);
        case OutRoute::MixW: return launch_apply_mix_w(R, I, a, *mix, ntiles, s, waves);
        default: return launch_apply(p->dtype, R, I, o.shared, a, ntiles, s);
    }
}

int psgd::compress_impl(psgd_plan* p, void* const* grads, int64_t step, int32_t it, hipStream_t s, StepCtx c) {
    if (it == 0) p->norm_rec.have = false;  // a new step: the recorded output terms are about to be overwritten
    if (p->f64()) return compress_f64(p, grads, step, it, s);
    if (p->wide()) return compress_wide(p, grads, step, it, s, c.xout);
    if (int st = refresh_pointers(p, grads, s)) return st;
    const Iter i{p, step, it, p->route(step, it, c), c.span ? *c.span : p->full_span(), s, c};
    if (int st = orth_stage(i)) return st;
    switch (i.r.pass) {
        case IterRoute::PassOddEven: return odd_even_stage(i);
        case IterRoute::PassFinal: return final_stage(i);
        default: return product_stage(i);
    }
}

// World-size-1 step (psgd_aggregate / psgd_aggregate_flat / psgd_aggregate_mixed): the rank-1 joint
// norm folded, the output written by the fused last iteration where the plan has one
int psgd::aggregate_ctx(psgd_plan* p, void* const* grads, int64_t step, hipStream_t s, StepCtx c) {
    c = world1_ctx(c);
    for (int it = 0; it < p->iters; ++it)
        if (int st = compress_impl(p, grads, step, it, s, c)) return st;
    return decompress_impl(p, grads, c.out, step, 1, s, c);
}

int psgd::decompress_impl(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world, hipStream_t s,
                          StepCtx c) {
    if (p->f64()) return decompress_f64(p, grads, out, step, world, s);
    if (p->wide()) return decompress_wide(p, grads, out, step, world, s);
    const OutRoute o = p->out_route(step, world, c);
    if (o.kind == OutRoute::None) return PSGD_OK;  // output written by the fused last iteration
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
    fill_terms(p, step, I, aa.apx, [&](int k) { return p->hist(0, k); },
               [&](int k) { return k + 1 < I ? p->hist(o.reduced_slot, k) : last; });
    aa.nterms = I;
    aa.alpha = float(1.0 / double(world));  // reference alpha = 1 / num_workers (:218)
    aa.ntiles = nt;
    if (c.fl && o.flat) aa.flat = *c.fl;  // uncompressed tensors (mixed_comm: their round items) ride in the launch
    if (nt + aa.flat.nitems == 0) return PSGD_OK;
    // for psgd_clip_outputs: the term set this pass reads (world size 1: the shared instance reads the
    // local terms alone, history slots 0 / 1, and never the state buffer)
    if (c.span == nullptr) p->record_terms(step, world, o.shared ? aa.res : aa.apx, I, aa.alpha);
    std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
    if (o.timed)
        if (int st = timing_begin(p, s, &ev, true)) return st;
    TimedScope ts(ev);
    PSGD_HIP(launch_out_pass(p, o, aa, c.mix, nt, s, nullptr, c.dst, c.fdst));
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
// collective: ingest-pack in a launch of its own first, the round items in the final launch.
// `mix` and `dst` (psgd_aggregate_mixed_comm_dst): `grads` already holds residual + gradients, so
// nothing is ingested: the flat tail is packed as psgd_aggregate_comm packs it (x / W, x = +0.0,
// flat_pack_item<float>), with mix->stage as its flat buffer, and the round items store into
// dst->unc_dst.
// `fdst` alone (psgd_aggregate_comm_dst): psgd_aggregate_comm's own sequence with fdst->stage where
// `flat_out` goes (packed by the same kernels: inside the first even product's launch, else
// flat_pack_item<float> in a launch of its own), the final pass's fp32 destination-table instance,
// and copy items (fdst->unc_dst = stage) as its leading workgroups
int psgd::aggregate_comm_ctx(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f,
                             void* const* unc, void* flat_out, psgd_comm* comm, hipStream_t s, const MixArgs* mix,
                             const MixDst* dst, const DirectDst* fdst) {
    const bool has_flat = f != nullptr;
    const int world = comm_world(comm);
    // x / W into the flat buffer, x = 0 (utils.py:43-47, powersgd.py:29-30): inside the first
    // even product's launch when the step starts even, else its own launch
    FlatArgs fa{};
    const bool ingest = mix && !dst;
    const bool fold = has_flat && !ingest && p->even(step, 0) && !p->wide();  // wide products carry no flat pack
    if (fdst) flat_out = fdst->stage;  // the collective's fp32 buffer; copy items follow it
    if (fold || ((mix || fdst) && has_flat)) {
        if (int st = flat_args(f, unc, dst ? static_cast<void*>(mix->stage) : flat_out, world, s, &fa)) return st;
        if (ingest) PSGD_HIP(launch_flat_ingest(fa, *mix, s));
        else if (!fold) PSGD_HIP(launch_flat_pack(f->dtype, fa, s));
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
    StepCtx d = comm_out_ctx(mix, dst);
    if (fdst) {  // the copy items ride in the final launch, whichever it is
        d.fdst = fdst;
        d.fl = has_flat ? &fa : nullptr;
    }
    if (!mix) return decompress_impl(p, grads, out, step, world, s, d);
    // the round items ride in every final launch built for them; a 1-rank communicator's unfused
    // final pass is the world-size-1 instance, whose flat items ingest: the round follows it
    const OutRoute o = p->out_route(step, world, d);
    const bool ride = o.kind == OutRoute::Lowrank || o.inst == OutRoute::MixW;
    d.fl = has_flat && ride ? &fa : nullptr;
    if (int st = decompress_impl(p, grads, out, step, world, s, d)) return st;
    if (has_flat && !ride) PSGD_HIP(dst ? launch_flat_round_dst(fa, *mix, dst->unc_dst, s) : launch_flat_round(fa, *mix, s));
    return PSGD_OK;
}

extern "C" {

int psgd_compress(psgd_plan* p, void* const* grads, int64_t step, int32_t it, void* stream) {
    if (int st = check_call(p && grads, p && p->bound, p && step >= 0 && it >= 0 && it < p->iters, "step/iteration out of range"))
        return st;
    DevScope scope(p->device);
    return compress_impl(p, grads, step, it, static_cast<hipStream_t>(stream), StepCtx{});
}

int psgd_decompress(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world,
                    void* stream) {
    if (int st = check_call(p && grads && out, p && p->bound, step >= 0 && world >= 1, "step/world size out of range"))
        return st;
    if (int st = check_out(out)) return st;
    DevScope scope(p->device);
    return decompress_impl(p, grads, out, step, world, static_cast<hipStream_t>(stream), StepCtx{});
}

int psgd_compress_bucket(psgd_plan* p, void* const* grads, int64_t step, int32_t it, int32_t bucket, void* stream) {
    if (int st = check_call(p && grads, p && p->bound, p && step >= 0 && it >= 0 && it < p->iters, "step/iteration out of range"))
        return st;
    psgd_plan::Span sp;
    if (int st = bucket_span(p, bucket, &sp)) return st;
    DevScope scope(p->device);
    StepCtx c;
    c.span = &sp;
    return compress_impl(p, grads, step, it, static_cast<hipStream_t>(stream), c);
}

int psgd_decompress_bucket(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world, int32_t bucket,
                           void* stream) {
    if (int st = check_call(p && grads && out, p && p->bound, step >= 0 && world >= 1, "step/world size out of range"))
        return st;
    if (int st = check_out(out)) return st;
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
    if (int st = check_call(p && grads && out, p && p->bound, step >= 0, "step out of range")) return st;
    if (int st = check_out(out)) return st;
    DevScope scope(p->device);
    StepCtx c;
    c.out = out;
    return aggregate_ctx(p, grads, step, static_cast<hipStream_t>(stream), c);
}

int psgd_aggregate_flat(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f,
                        void* const* unc, void* flat_out, void* stream) {
    if (!f || f->total == 0) return psgd_aggregate(p, grads, out, step, stream);
    if (int st = check_call(p && grads && out && unc && flat_out, p && p->bound && f->bound, step >= 0, "step out of range"))
        return st;
    if (int st = check_out(out)) return st;
    if (f->dtype != p->dtype || f->device != p->device || p->f64() || p->wide()) {  // separate launches
        if (int st = psgd_aggregate(p, grads, out, step, stream)) return st;
        return psgd_flat_pack(f, unc, flat_out, 1, stream);
    }
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FlatArgs a;
    if (int st = flat_args(f, unc, flat_out, 1, s, &a)) return st;
    StepCtx c;
    c.fl = &a;
    c.out = out;
    return aggregate_ctx(p, grads, step, s, c);
}

// World size W in one call (include/psgd.h): per iteration the kernels, then the in-place SUM
// all-reduce of the out-factor state on the same stream (the last grouped with the flat
// buffer of the uncompressed tensors), then the output pass. Same sequence as the building
// blocks psgd_compress / all_reduce / psgd_decompress (reference powersgd.py:172-230).
int psgd_aggregate_comm(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f, void* const* unc,
                        void* flat_out, psgd_comm* comm, void* stream) {
    if (int st = check_call(p && grads && out && comm, p && p->bound, step >= 0, "step out of range")) return st;
    if (p->f64()) return fail(PSGD_ERR_DTYPE, "psgd_aggregate_comm takes fp32/bf16 plans (fp32 factors)");
    if (int st = check_out(out)) return st;
    const bool has_flat = f && f->total > 0;
    if (has_flat)
        if (int st = check_flat(f, unc && flat_out, f->dtype == PSGD_F32, PSGD_ERR_DTYPE,
                                "psgd_aggregate_comm packs fp32 uncompressed tensors"))
            return st;
    // a poisoned communicator is refused before the step launches anything: the caller's
    // gradients and the P/Q state stay as they were
    std::string why;
    if (comm_poisoned(comm, &why))
        return fail(PSGD_ERR_STATE, ("communicator unusable after an earlier failure: " + why).c_str());
    DevScope scope(p->device);
    const int st = aggregate_comm_ctx(p, grads, out, step, has_flat ? f : nullptr, unc, flat_out, comm,
                                      static_cast<hipStream_t>(stream), nullptr);
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
