// psgd_adam_update / psgd_adam_update_mp (include/psgd.h) and the device tables of psgd_aggregate_comm_adam's sink, as
// psgd_sgd.cpp keeps the SGD ones: a state of the plan's own (psgd_plan::Adam) with word tables
// (psgd_tables.h). Pointers and work items are one table, the records another: bias correction
// changes the records every step, so a step uploads them alone (an async copy on the codec's stream
// from the cache's pinned staging; the host does not wait for the stream).
#include "psgd_tables.h"

using psgd::put;
using psgd::put_ptrs;
using psgd::WordTable;

static_assert(sizeof(psgd_adam_hyper) == 9 * sizeof(float), "records are dense: hyper[i] on the device is the host's");

struct psgd_plan::Adam {
    WordTable upd_tab, upd_hyper;    // psgd_adam_update: pointers + work items; records
    WordTable sink_tab, sink_hyper;  // psgd_aggregate_comm_adam: the sink's pointer tables; records
    float* stage = nullptr;          // fp32 stage of the flat tail (the flat plan's layout)
    size_t stage_cap = 0;
    std::vector<void*> words;  // scratch of a call: nothing is allocated once it has its size
    // the master-weight forms (psgd_adam_update_mp, psgd_aggregate_mixed_comm_adam): tables of their
    // own, so a plan that mixes both forms re-binds nothing; and the ADD of the flat plan's tensors
    // (bf16 gradients into their fp32 residual), a run table over that plan's element counts
    WordTable mp_tab, mp_hyper, sink_w;
    psgd::FlatAdd unc_add;
    ~Adam() {
        if (stage) (void)hipFree(stage);
    }
};

namespace psgd {

void adam_release(psgd_plan* p) {
    delete p->adam;
    p->adam = nullptr;
}

int adam_check(const psgd_plan* p, void* const* ms, void* const* vs, const psgd_flat* f, void* const* unc_ms,
               void* const* unc_vs) {
    const size_t nt = p->shapes.size(), nu = f ? size_t(f->count) : 0;
    if (nu && (!unc_ms || !unc_vs)) return fail(PSGD_ERR_VALUE, "null moment table of the flat plan's tensors");
    for (size_t i = 0; i < nt + nu; ++i) {
        void* const m = i < nt ? ms[i] : unc_ms[i - nt];
        void* const v = i < nt ? vs[i] : unc_vs[i - nt];
        if (!m || !v) return fail(PSGD_ERR_VALUE, "null moment (exp_avg / exp_avg_sq) pointer");
        if ((reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) % 4)
            return fail(PSGD_ERR_LAYOUT, "moments must be 4-byte aligned");
    }
    return PSGD_OK;
}

int adam_select(psgd_plan* p, void* const* params, void* const* ms, void* const* vs, const psgd_flat* f,
                void* const* unc_params, void* const* unc_ms, void* const* unc_vs, const psgd_adam_hyper* hyper,
                hipStream_t s, OutSink* sink) {
    if (!p->adam) p->adam = new psgd_plan::Adam();
    psgd_plan::Adam& m = *p->adam;
    const size_t nt = p->shapes.size(), nu = f ? size_t(f->count) : 0;
    if (f && size_t(f->total) > m.stage_cap) {
        PSGD_HIP(hipStreamSynchronize(s));
        if (m.stage) PSGD_HIP(hipFree(m.stage));
        m.stage = nullptr;
        m.stage_cap = 0;
        PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&m.stage), size_t(f->total) * sizeof(float)));
        m.stage_cap = size_t(f->total);
    }
    std::vector<void*>& w = m.words;
    w.clear();
    put_ptrs(w, params, nt);
    put_ptrs(w, ms, nt);
    put_ptrs(w, vs, nt);
    put_ptrs(w, unc_params, nu);
    put_ptrs(w, unc_ms, nu);
    put_ptrs(w, unc_vs, nu);
    const void* tab = nullptr;
    if (int st = m.sink_tab.select(w, s, &tab)) return st;
    void* const* t = static_cast<void* const*>(tab);
    w.clear();
    put(w, hyper, (nt + nu) * sizeof(psgd_adam_hyper));
    const void* hy = nullptr;
    if (int st = m.sink_hyper.select(w, s, &hy)) return st;
    sink->adam = sink->tables = true;
    sink->dst = t;
    sink->bufs = t + nt;
    sink->vs = t + 2 * nt;
    sink->unc_dst = t + 3 * nt;
    sink->unc_bufs = t + 3 * nt + nu;
    sink->unc_vs = t + 3 * nt + 2 * nu;
    sink->adam_hyper = static_cast<const psgd_adam_hyper*>(hy);
    sink->hyper_unc0 = int32_t(nt);
    sink->stage = f ? m.stage : nullptr;
    return PSGD_OK;
}

int adam_mp_check(const psgd_plan* p, void* const* grads16, void* const* ws, const psgd_flat* f, void* const* unc16,
                  void* const* unc_ws) {
    const size_t nt = p->shapes.size(), nu = f ? size_t(f->count) : 0;
    if (nu && (!unc16 || !unc_ws)) return fail(PSGD_ERR_VALUE, "null bf16 table of the flat plan's tensors");
    for (size_t i = 0; i < nt + nu; ++i) {
        void* const g = i < nt ? grads16[i] : unc16[i - nt];
        void* const w = i < nt ? ws[i] : unc_ws[i - nt];
        if (!g || !w) return fail(PSGD_ERR_VALUE, "null bf16 gradient or model parameter pointer");
        if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(w)) % 2)
            return fail(PSGD_ERR_LAYOUT, "bf16 gradients and model parameters must be 2-byte aligned");
    }
    return PSGD_OK;
}

int adam_mp_add(psgd_plan* p, const psgd_flat* f, void* const* unc16, void* const* unc_residual, hipStream_t s) {
    if (!f) return PSGD_OK;
    if (!p->adam) p->adam = new psgd_plan::Adam();
    return p->adam->unc_add.add(p->device, f, unc16, unc_residual, s);
}

int adam_mp_select(psgd_plan* p, void* const* ws, const psgd_flat* f, void* const* unc_ws, hipStream_t s, OutSink* sink) {
    psgd_plan::Adam& m = *p->adam;  // after adam_select
    const size_t nt = p->shapes.size(), nu = f ? size_t(f->count) : 0;
    std::vector<void*>& w = m.words;
    w.clear();
    put_ptrs(w, ws, nt);
    put_ptrs(w, unc_ws, nu);
    const void* tab = nullptr;
    if (int st = m.sink_w.select(w, s, &tab)) return st;
    void* const* t = static_cast<void* const*>(tab);
    sink->adam_mp = true;
    sink->ws = t;
    sink->unc_ws = t + nt;
    return PSGD_OK;
}

}  // namespace psgd

using namespace psgd;

// psgd_adam_update (`mp` false: w unused) and psgd_adam_update_mp (w[i] = bf16(p'[i]))
static int adam_update_any(psgd_plan* plan, int32_t count, void* const* g, void* const* p, void* const* mo,
                           void* const* v, void* const* wt, bool mp, const int64_t* numel, const psgd_adam_hyper* hyper,
                           void* stream) {
    if (!g || !p || !mo || !v || (mp && !wt) || !numel || !hyper || count < 1) return fail(PSGD_ERR_VALUE, "null argument");
    if (plan && !plan->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    const size_t n = size_t(count);
    size_t nitems = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!g[i] || !p[i]) return fail(PSGD_ERR_VALUE, "null tensor pointer");
        if (!mo[i] || !v[i]) return fail(PSGD_ERR_VALUE, "null moment (exp_avg / exp_avg_sq) pointer");
        if (mp && !wt[i]) return fail(PSGD_ERR_VALUE, "null bf16 model parameter pointer");
        if (numel[i] < 0) return fail(PSGD_ERR_VALUE, "negative element count");
        nitems += size_t((numel[i] + kRunItem - 1) / kRunItem);
    }
    for (size_t i = 0; i < n; ++i) {
        const uintptr_t all = reinterpret_cast<uintptr_t>(g[i]) | reinterpret_cast<uintptr_t>(p[i]) |
                              reinterpret_cast<uintptr_t>(mo[i]) | reinterpret_cast<uintptr_t>(v[i]);
        if (all % 4) return fail(PSGD_ERR_LAYOUT, "averages, weights and moments must be 4-byte aligned");
        if (mp && reinterpret_cast<uintptr_t>(wt[i]) % 2)
            return fail(PSGD_ERR_LAYOUT, "bf16 model parameters must be 2-byte aligned");
    }
    if (nitems == 0) return PSGD_OK;
    if (nitems > size_t(INT32_MAX)) return fail(PSGD_ERR_VALUE, "too many work items");
    hipStream_t s = static_cast<hipStream_t>(stream);
    psgd_plan::Adam local;  // no plan: a state of this call
    if (plan && !plan->adam) plan->adam = new psgd_plan::Adam();
    psgd_plan::Adam& m = plan ? *plan->adam : local;
    DevScope scope(plan ? plan->device : -1);
    // words: [g][p][m][v][items], the master-weight form [w] ahead of them
    std::vector<void*>& w = m.words;
    w.clear();
    if (mp) put_ptrs(w, wt, n);
    put_ptrs(w, g, n);
    put_ptrs(w, p, n);
    put_ptrs(w, mo, n);
    put_ptrs(w, v, n);
    std::vector<SgdItem> items;
    items.reserve(nitems);
    for (size_t i = 0; i < n; ++i)
        for (int64_t o = 0; o < numel[i]; o += kRunItem)
            items.push_back(SgdItem{o, int32_t(i), int32_t(std::min<int64_t>(kRunItem, numel[i] - o))});
    put(w, items.data(), items.size() * sizeof(SgdItem));
    const void* tab = nullptr;
    if (int st = (mp ? m.mp_tab : m.upd_tab).select(w, s, &tab)) return st;
    w.clear();
    put(w, hyper, n * sizeof(psgd_adam_hyper));
    const void* hy = nullptr;
    if (int st = (mp ? m.mp_hyper : m.upd_hyper).select(w, s, &hy)) return st;
    void* const* t = static_cast<void* const*>(tab) + (mp ? n : 0);
    AdamArgs a{};
    a.g = t;
    a.p = t + n;
    a.m = t + 2 * n;
    a.v = t + 3 * n;
    a.items = reinterpret_cast<const SgdItem*>(t + 4 * n);
    a.hyper = static_cast<const psgd_adam_hyper*>(hy);
    a.nitems = int32_t(nitems);
    if (mp) PSGD_HIP(launch_adam_update_mp(AdamMpArgs{a, static_cast<void* const*>(tab)}, s));
    else PSGD_HIP(launch_adam_update(a, s));
    if (!plan) PSGD_HIP(hipStreamSynchronize(s));  // `local` (tables, pinned staging) goes with the call
    return PSGD_OK;
}

extern "C" int psgd_adam_update(psgd_plan* plan, int32_t count, void* const* g, void* const* p, void* const* mo,
                                void* const* v, const int64_t* numel, const psgd_adam_hyper* hyper, void* stream) {
    return adam_update_any(plan, count, g, p, mo, v, nullptr, false, numel, hyper, stream);
}

extern "C" int psgd_adam_update_mp(psgd_plan* plan, int32_t count, void* const* g, void* const* p, void* const* mo,
                                   void* const* v, void* const* w_bf16, const int64_t* numel,
                                   const psgd_adam_hyper* hyper, void* stream) {
    return adam_update_any(plan, count, g, p, mo, v, w_bf16, true, numel, hyper, stream);
}
