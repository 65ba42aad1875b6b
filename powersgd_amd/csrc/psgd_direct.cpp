// psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst / psgd_plan_dst_ok (include/psgd.h): the default
// (fp32) DDP hook's one-call completion. Defined as, and bit for bit equal to,
//   psgd_aggregate_comm (psgd_aggregate_ipc) on the gradients
//   dst[i][e] = out_i[e], unc_dst[k][e] = flat_k[e]     (the per-bucket psgd_runs_gather)
// with the same kernels in the same order and the same collectives or exchanges: the final pass is
// its fp32 destination-table instance (psgd_apply_dst.hip, DirectDst) and stores every average at
// the tensor's own destination, so no output slab is written and no gather runs. The flat tail's
// collective (or last exchange) sums into a staging buffer of the plan's own, passed where
// flat_out goes; copy items (unc_dst[k] = stage) are the leading workgroups of the final launch.
// Eligible: an fp32 plan, not wide, one bucket, every destination-table instance the plan's
// routes name admitted (two waves per SIMD, no scratch) for both step parities and both
// communicator kinds.
#include <memory>
#include <string>

#include "psgd_plan.h"

namespace {

const char* ineligible(const psgd_plan* p, int* code) {
    *code = PSGD_ERR_VALUE;
    if (p->dtype != PSGD_F32) {
        *code = PSGD_ERR_DTYPE;
        return "psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst take an fp32 plan";
    }
    if (p->wide()) return "psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst serve rank buckets 1 to 32";
    if (p->spans.size() > 1) return "psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst take a plan of one bucket";
    return nullptr;
}

StepCtx out_ctx(const DirectDst* t) {
    StepCtx c;
    c.fdst = t;
    return c;
}

// Admission: the runtime keeps at least two waves per SIMD of the destination-table instance a
// route's output pass would launch, without scratch. Asked through launch_out_pass, the function
// the drivers launch with. The routes read fin_ok and out_nt of what a re-tiling can change: the
// key (the sibling's admit_dst has one of its own)
void admit(psgd_plan* p) {
    psgd_plan::Direct& m = *p->direct;
    const uint64_t key = uint64_t(p->fin_ok) | uint64_t(uint32_t(p->out_nt)) << 8;
    if (m.key == key) return;
    m.key = key;
    const DirectDst tabs{};
    for (int one = 0; one < 2; ++one)
        for (int par = 0; par < 2; ++par) {
            int w = 0;
            ApplyArgs aa{};
            const OutRoute o = p->out_route(par, one ? 1 : 2, out_ctx(&tabs));
            const hipError_t e = launch_out_pass(p, o, aa, nullptr, 0, nullptr, &w, nullptr, &tabs);
            m.ok[one][par] = e == hipSuccess && w >= 2;
        }
}

// every instance, both parities, both communicator kinds: a property of the plan
bool eligible(const psgd_plan* p) {
    const psgd_plan::Direct& m = *p->direct;
    return m.ok[0][0] && m.ok[0][1] && m.ok[1][0] && m.ok[1][1];
}

// The plan's direct-store state: the destinations' pointer tables, device side in one allocation
// of the plan's own (made once, by the first call on a bound plan)
int ensure(psgd_plan* p) {
    if (p->direct) return PSGD_OK;
    std::unique_ptr<psgd_plan::Direct> m(new psgd_plan::Direct());
    const size_t nt = p->shapes.size();
    PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&m->dev), TableCache::bytes(nt)));
    m->dst.bind(m->dev, nt);
    p->direct = m.release();
    return PSGD_OK;
}

// room for the uncompressed tensors' destination table and the fp32 staging of the flat tail
// (first call, or a larger flat plan than the last one's)
int flat_room(psgd_plan::Direct& m, const psgd_flat* f, hipStream_t s) {
    const size_t cnt = size_t(f->count);
    if (cnt > m.unc_cap) {
        PSGD_HIP(hipStreamSynchronize(s));
        m.unc_dst.release();
        if (m.unc_dev) PSGD_HIP(hipFree(m.unc_dev));
        m.unc_dev = nullptr;
        m.unc_cap = 0;
        PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&m.unc_dev), TableCache::bytes(cnt)));
        m.unc_cap = cnt;
        m.unc_dst.bind(m.unc_dev, cnt);
    } else if (m.unc_dst.n != cnt) {
        PSGD_HIP(hipStreamSynchronize(s));
        m.unc_dst.bind(m.unc_dev, cnt);
    }
    if (size_t(f->total) > m.stage_cap) {
        PSGD_HIP(hipStreamSynchronize(s));
        if (m.stage) PSGD_HIP(hipFree(m.stage));
        m.stage = nullptr;
        m.stage_cap = 0;
        PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&m.stage), size_t(f->total) * sizeof(float)));
        m.stage_cap = size_t(f->total);
    }
    return PSGD_OK;
}

// what both entry points check of their arguments, before the plan's device state: the plan's
// eligibility by shape, the flat plan, every tensor's two pointers and the uncompressed tensors'
int check_args(const psgd_plan* p, void* const* grads, void* const* dst, const psgd_flat* f, void* const* unc,
               void* const* unc_dst, const char* who) {
    int code = PSGD_ERR_VALUE;
    if (const char* why = ineligible(p, &code)) return fail(code, why);
    if (f) {
        if (int st = check_flat(f, unc && unc_dst, f->dtype == PSGD_F32 && f->device == p->device, PSGD_ERR_VALUE,
                                (std::string(who) + " takes an fp32 flat plan on the codec's device").c_str()))
            return st;
        for (int32_t i = 0; i < f->count; ++i)
            if (!unc[i] || !unc_dst[i]) return fail(PSGD_ERR_VALUE, "null uncompressed tensor pointer");
    }
    for (size_t i = 0; i < p->shapes.size(); ++i) {
        if (!grads[i] || !dst[i]) return fail(PSGD_ERR_VALUE, "null gradient pointer");
        if (reinterpret_cast<uintptr_t>(dst[i]) % 4) return fail(PSGD_ERR_LAYOUT, "fp32 destinations must be 4-byte aligned");
    }
    if (f)
        for (int32_t i = 0; i < f->count; ++i)
            if (reinterpret_cast<uintptr_t>(unc_dst[i]) % 4)
                return fail(PSGD_ERR_LAYOUT, "fp32 destinations must be 4-byte aligned");
    return PSGD_OK;
}

// Past the argument checks: the state, the tiling the step will run on (the gradients' alignment
// decides the vector layout, as in the three-stage flow; the destinations' only picks the store
// form, in the kernel), admission, then the tables. *refused: nothing was launched
int prepare(psgd_plan* p, void* const* grads, void* const* dst, psgd_flat* f, void* const* unc_dst, hipStream_t s,
            const char* who, DirectDst* t, bool* refused) {
    if (int st = ensure(p)) return st;
    psgd_plan::Direct& m = *p->direct;
    if (int st = refresh_pointers(p, grads, s)) return st;
    admit(p);
    if (!eligible(p)) {
        *refused = true;
        return fail(PSGD_ERR_VALUE, std::string(who) + ": a destination-table instance of this plan's final pass is not "
                                                       "admitted (two waves per SIMD, no scratch)");
    }
    if (f) {
        if (int st = flat_room(m, f, s)) return st;
        PSGD_HIP(m.unc_dst.select(unc_dst, s));
        t->unc_dst = m.unc_dst.table();
        t->stage = m.stage;
    }
    PSGD_HIP(m.dst.select(dst, s));
    t->dst = m.dst.table();
    return PSGD_OK;
}

}  // namespace

bool psgd::direct_shape_ok(const psgd_plan* p) {
    int code = 0;
    return ineligible(p, &code) == nullptr;
}

int psgd::direct_select(psgd_plan* p, void* const* dst, const psgd_flat* f, void* const* unc_dst, hipStream_t s,
                        DirectDst* t) {
    if (f) {  // checked before the state is made: a refusal leaves nothing behind
        const psgd_plan::Direct* m = p->direct;
        if (!m || !m->stage || m->stage_cap < size_t(f->total) || m->unc_cap < size_t(f->count))
            return fail(PSGD_ERR_STATE, "the flat tail is not staged (call after psgd_aggregate_comm_dst / _ipc_dst)");
    }
    if (int st = ensure(p)) return st;
    psgd_plan::Direct& m = *p->direct;
    if (f) {
        if (m.unc_dst.n != size_t(f->count)) {
            PSGD_HIP(hipStreamSynchronize(s));
            m.unc_dst.bind(m.unc_dev, size_t(f->count));
        }
        PSGD_HIP(m.unc_dst.select(unc_dst, s));
        t->unc_dst = m.unc_dst.table();
        t->stage = m.stage;
    }
    PSGD_HIP(m.dst.select(dst, s));
    t->dst = m.dst.table();
    return PSGD_OK;
}

void psgd::direct_release(psgd_plan* p) {
    if (!p->direct) return;
    psgd_plan::Direct* m = p->direct;
    m->dst.release();
    m->unc_dst.release();
    if (m->dev) (void)hipFree(m->dev);
    if (m->unc_dev) (void)hipFree(m->unc_dev);
    if (m->stage) (void)hipFree(m->stage);
    delete m;
    p->direct = nullptr;
}

extern "C" {

int psgd_plan_dst_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok) {
    if (!plan || !ok) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (world < 1) return fail(PSGD_ERR_VALUE, "world size must be >= 1");
    *ok = 0;
    int code = 0;
    if (ineligible(plan, &code)) return PSGD_OK;
    // admission is a property of this build's kernels on the device: asked once per tiling and
    // cached in the plan; a plan with no device yet asks without keeping device state
    psgd_plan* p = const_cast<psgd_plan*>(plan);
    DevScope scope(p->device);
    psgd_plan::Direct tmp;
    const bool unbound = !p->direct && !p->bound;
    if (unbound) p->direct = &tmp;
    if (!p->direct)
        if (int st = ensure(p)) return st;
    admit(p);
    *ok = eligible(p) ? 1 : 0;
    if (unbound) p->direct = nullptr;
    return PSGD_OK;
}

int psgd_aggregate_comm_dst(psgd_plan* p, void* const* grads, void* const* dst, int64_t step, psgd_flat* f,
                            void* const* unc, void* const* unc_dst, psgd_comm* comm, void* stream) {
    if (int st = check_call(p && grads && dst && comm, p && p->bound, step >= 0, "step out of range")) return st;
    const bool has_flat = f && f->total > 0;
    if (int st = check_args(p, grads, dst, has_flat ? f : nullptr, unc, unc_dst, "psgd_aggregate_comm_dst")) return st;
    // a poisoned communicator is refused before the step launches anything: the caller's
    // gradients, the destinations and the P/Q state stay as they were
    std::string why;
    if (comm_poisoned(comm, &why))
        return fail(PSGD_ERR_STATE, ("communicator unusable after an earlier failure: " + why).c_str());
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DirectDst t{};
    bool refused = false;
    int st = prepare(p, grads, dst, has_flat ? f : nullptr, unc_dst, s, "psgd_aggregate_comm_dst", &t, &refused);
    if (!st) st = aggregate_comm_ctx(p, grads, nullptr, step, has_flat ? f : nullptr, unc, nullptr, comm, s, nullptr, nullptr, &t);
    // a failure past the argument checks can leave this rank's collective sequence short of its
    // peers': the communicator refuses every later call (psgd_comm.cpp, comm_poison)
    if (st && !refused) comm_poison(comm, psgd_last_error());
    return st;
}

int psgd_aggregate_ipc_dst(psgd_plan* p, void* const* grads, void* const* dst, int64_t step, psgd_flat* f,
                           void* const* unc, void* const* unc_dst, void* stream) {
    // the argument errors (null, a negative step) before the plan's state
    if (!p || !grads || !dst) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    const bool has_flat = f && f->total > 0;
    if (int st = check_args(p, grads, dst, has_flat ? f : nullptr, unc, unc_dst, "psgd_aggregate_ipc_dst")) return st;
    if (int st = ipc_check(p, step)) return st;
    if (has_flat && f->total > p->ipc_flat_cap)
        return fail(PSGD_ERR_VALUE, "flat tensors exceed the exchange buffer (psgd_ipc_create)");
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DirectDst t{};
    bool refused = false;
    if (int st = prepare(p, grads, dst, has_flat ? f : nullptr, unc_dst, s, "psgd_aggregate_ipc_dst", &t, &refused))
        return st;
    return aggregate_ipc_ctx(p, grads, nullptr, step, has_flat ? f : nullptr, unc, nullptr, s, nullptr, nullptr, &t);
}

}  // extern "C"
