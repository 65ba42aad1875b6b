// psgd_sgd_update / psgd_sgd_update_mp (include/psgd.h) and the device tables of psgd_aggregate_comm_sgd's sink. Both keep
// their tables in a state of the plan's own (psgd_plan::Sgd, like Guard): word tables, a
// TableCache over 8-byte words with a device allocation that grows on demand. What rarely changes
// (pointers, work items) and what a learning-rate schedule changes every step (the records) are
// tables of their own, so a step with a new learning rate uploads the records alone: an async copy
// on the codec's stream from the cache's pinned staging. The host does not wait for the stream;
// TableCache::select does wait on the event of the upload that last used the slot it reuses (four
// misses earlier under a schedule: a copy of a few KiB, long complete, so the wait returns at once).
#include <cstring>

#include "psgd_tables.h"

using psgd::put;
using psgd::put_ptrs;
using psgd::WordTable;

namespace {

static_assert(sizeof(psgd_sgd_hyper) == 3 * sizeof(void*), "a record is three table words");
static_assert(sizeof(psgd::SgdItem) == 2 * sizeof(void*), "a work item is two table words");

}  // namespace

struct psgd_plan::Sgd {
    WordTable upd_tab, upd_hyper;  // psgd_sgd_update: pointers + work items; records
    WordTable sink_tab, sink_hyper;  // psgd_aggregate_comm_sgd: the sink's pointer tables; records
    float* stage = nullptr;  // fp32 stage of the flat tail (the flat plan's layout)
    size_t stage_cap = 0;
    std::vector<void*> words;  // scratch of a call: nothing is allocated once it has its size
    // the master-weight forms (psgd_sgd_update_mp, psgd_aggregate_mixed_comm_sgd): tables of their
    // own, so a plan that mixes both forms re-binds nothing; and the ADD of the flat plan's tensors
    WordTable mp_tab, mp_hyper, sink_w;
    psgd::FlatAdd unc_add;
    ~Sgd() {
        if (stage) (void)hipFree(stage);
    }
};

namespace psgd {

void sgd_release(psgd_plan* p) {
    delete p->sgd;
    p->sgd = nullptr;
}

int sgd_check(const psgd_plan* p, void* const* bufs, const psgd_flat* f, void* const* unc_bufs,
              const psgd_sgd_hyper* hyper) {
    const size_t nt = p->shapes.size(), nu = f ? size_t(f->count) : 0;
    for (size_t i = 0; i < nt + nu; ++i) {
        void* const b = i < nt ? (bufs ? bufs[i] : nullptr) : (unc_bufs ? unc_bufs[i - nt] : nullptr);
        if (hyper[i].momentum != 0.f && !b) return fail(PSGD_ERR_VALUE, "null momentum buffer of a tensor with momentum");
        if (reinterpret_cast<uintptr_t>(b) % 4) return fail(PSGD_ERR_LAYOUT, "momentum buffers must be 4-byte aligned");
    }
    return PSGD_OK;
}

int sgd_select(psgd_plan* p, void* const* params, void* const* bufs, const psgd_flat* f, void* const* unc_params,
               void* const* unc_bufs, const psgd_sgd_hyper* hyper, hipStream_t s, OutSink* sink) {
    if (!p->sgd) p->sgd = new psgd_plan::Sgd();
    psgd_plan::Sgd& m = *p->sgd;
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
    put_ptrs(w, bufs, nt);
    put_ptrs(w, unc_params, nu);
    put_ptrs(w, unc_bufs, nu);
    const void* tab = nullptr;
    if (int st = m.sink_tab.select(w, s, &tab)) return st;
    void* const* t = static_cast<void* const*>(tab);
    w.clear();
    put(w, hyper, (nt + nu) * sizeof(psgd_sgd_hyper));
    const void* hy = nullptr;
    if (int st = m.sink_hyper.select(w, s, &hy)) return st;
    sink->sgd = sink->tables = true;
    sink->dst = t;
    sink->bufs = t + nt;
    sink->unc_dst = t + 2 * nt;
    sink->unc_bufs = t + 2 * nt + nu;
    sink->hyper = static_cast<const psgd_sgd_hyper*>(hy);
    sink->hyper_unc0 = int32_t(nt);
    sink->stage = f ? m.stage : nullptr;
    return PSGD_OK;
}

int sgd_mp_add(psgd_plan* p, const psgd_flat* f, void* const* unc16, void* const* unc_residual, hipStream_t s) {
    if (!f) return PSGD_OK;
    return p->sgd->unc_add.add(p->device, f, unc16, unc_residual, s);  // after sgd_select
}

int sgd_mp_select(psgd_plan* p, void* const* ws, const psgd_flat* f, void* const* unc_ws, hipStream_t s, OutSink* sink) {
    psgd_plan::Sgd& m = *p->sgd;  // after sgd_select
    const size_t nt = p->shapes.size(), nu = f ? size_t(f->count) : 0;
    std::vector<void*>& w = m.words;
    w.clear();
    put_ptrs(w, ws, nt);
    put_ptrs(w, unc_ws, nu);
    const void* tab = nullptr;
    if (int st = m.sink_w.select(w, s, &tab)) return st;
    void* const* t = static_cast<void* const*>(tab);
    sink->sgd_mp = true;
    sink->ws = t;
    sink->unc_ws = t + nt;
    return PSGD_OK;
}

}  // namespace psgd

using namespace psgd;

// psgd_sgd_update (`mp` false: w unused) and psgd_sgd_update_mp (w[i] = bf16(p'[i]))
static int sgd_update_any(psgd_plan* plan, int32_t count, void* const* g, void* const* p, void* const* buf,
                          void* const* wt, bool mp, const int64_t* numel, const psgd_sgd_hyper* hyper, void* stream) {
    if (!g || !p || (mp && !wt) || !numel || !hyper || count < 1) return fail(PSGD_ERR_VALUE, "null argument");
    if (plan && !plan->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    const size_t n = size_t(count);
    size_t nitems = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!g[i] || !p[i]) return fail(PSGD_ERR_VALUE, "null tensor pointer");
        if (mp && !wt[i]) return fail(PSGD_ERR_VALUE, "null bf16 model parameter pointer");
        if (hyper[i].momentum != 0.f && (!buf || !buf[i]))
            return fail(PSGD_ERR_VALUE, "null momentum buffer of a tensor with momentum");
        if (numel[i] < 0) return fail(PSGD_ERR_VALUE, "negative element count");
        nitems += size_t((numel[i] + kRunItem - 1) / kRunItem);
    }
    for (size_t i = 0; i < n; ++i) {
        const uintptr_t all = reinterpret_cast<uintptr_t>(g[i]) | reinterpret_cast<uintptr_t>(p[i]) |
                              reinterpret_cast<uintptr_t>(buf ? buf[i] : nullptr);
        if (all % 4) return fail(PSGD_ERR_LAYOUT, "averages, weights and momentum buffers must be 4-byte aligned");
        if (mp && reinterpret_cast<uintptr_t>(wt[i]) % 2)
            return fail(PSGD_ERR_LAYOUT, "bf16 model parameters must be 2-byte aligned");
    }
    if (nitems == 0) return PSGD_OK;
    if (nitems > size_t(INT32_MAX)) return fail(PSGD_ERR_VALUE, "too many work items");
    hipStream_t s = static_cast<hipStream_t>(stream);
    psgd_plan::Sgd local;  // no plan: a state of this call
    if (plan && !plan->sgd) plan->sgd = new psgd_plan::Sgd();
    psgd_plan::Sgd& m = plan ? *plan->sgd : local;
    DevScope scope(plan ? plan->device : -1);
    // words: [g][p][buf][items], the master-weight form [w] ahead of them
    std::vector<void*>& w = m.words;
    w.clear();
    if (mp) put_ptrs(w, wt, n);
    put_ptrs(w, g, n);
    put_ptrs(w, p, n);
    put_ptrs(w, buf, n);
    std::vector<SgdItem> items;
    items.reserve(nitems);
    for (size_t i = 0; i < n; ++i)
        for (int64_t o = 0; o < numel[i]; o += kRunItem)
            items.push_back(SgdItem{o, int32_t(i), int32_t(std::min<int64_t>(kRunItem, numel[i] - o))});
    put(w, items.data(), items.size() * sizeof(SgdItem));
    const void* tab = nullptr;
    if (int st = (mp ? m.mp_tab : m.upd_tab).select(w, s, &tab)) return st;
    w.clear();
    put(w, hyper, n * sizeof(psgd_sgd_hyper));
    const void* hy = nullptr;
    if (int st = (mp ? m.mp_hyper : m.upd_hyper).select(w, s, &hy)) return st;
    void* const* t = static_cast<void* const*>(tab) + (mp ? n : 0);
    SgdArgs a{};
    a.g = t;
    a.p = t + n;
    a.buf = t + 2 * n;
    a.items = reinterpret_cast<const SgdItem*>(t + 3 * n);
    a.hyper = static_cast<const psgd_sgd_hyper*>(hy);
    a.nitems = int32_t(nitems);
    if (mp) PSGD_HIP(launch_sgd_update_mp(SgdMpArgs{a, static_cast<void* const*>(tab)}, s));
    else PSGD_HIP(launch_sgd_update(a, s));
    if (!plan) PSGD_HIP(hipStreamSynchronize(s));  // `local` (tables, pinned staging) goes with the call
    return PSGD_OK;
}

extern "C" int psgd_sgd_update(psgd_plan* plan, int32_t count, void* const* g, void* const* p, void* const* buf,
                               const int64_t* numel, const psgd_sgd_hyper* hyper, void* stream) {
    return sgd_update_any(plan, count, g, p, buf, nullptr, false, numel, hyper, stream);
}

extern "C" int psgd_sgd_update_mp(psgd_plan* plan, int32_t count, void* const* g, void* const* p, void* const* buf,
                                  void* const* w_bf16, const int64_t* numel, const psgd_sgd_hyper* hyper, void* stream) {
    return sgd_update_any(plan, count, g, p, buf, w_bf16, true, numel, hyper, stream);
}
