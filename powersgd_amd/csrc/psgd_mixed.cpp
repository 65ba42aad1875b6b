// psgd_aggregate_mixed / psgd_aggregate_mixed_flat / psgd_plan_mixed_folds (include/psgd.h): the
// world-size-1 step of an fp32 plan on an fp32 error-feedback residual fed by bf16 gradients, with
// the element-wise passes around the codec folded into its own gradient passes (MixArgs,
// psgd_internal.h). Defined as, and bit for bit equal to,
//   residual += float(g); g = +0.0        (psgd_runs_add_list, zero_source)
//   psgd_aggregate[_flat] on the residual
//   out = bf16(averages)                  (psgd_runs_gather)
// Which passes fold on a step:
//   output fold  always (the plan is eligible only when the final pass of either step parity has
//                an admitted mixed instance: there is no fp32 output buffer to fall back to)
//   ingest fold  when the step's only gradient pass is the single-pass k_final_odd (I = 1, odd
//                step, ranks 1 / 2) and that mixed instance is admitted; every other step runs the
//                run-table ADD as a launch of its own first (first pass k_even: the fold was built
//                and measured slower than the ADD it replaces; k_final_oe
//                and the unfused odd product: no fold built)
// psgd_aggregate_mixed_comm / psgd_plan_mixed_folds_comm: the same at world size W over a
// communicator, defined as the ADD, psgd_aggregate_comm on the residual and the GATHER. The output
// fold alone, on every step (admission per communicator kind, admit_comm); the ADD is always a
// launch of its own, first; the flat tail is staged in fp32 (Mixed::stage) around its collective.
// psgd_aggregate_mixed_comm_dst / psgd_plan_mixed_folds_dst: the DDP hook's form of the same step.
// The residual already holds residual + gradients (the hook adds each bucket on arrival), so the
// call is psgd_aggregate_comm on the residual and the GATHER alone, and the final pass stores each
// tensor's bf16 average at the tensor's own destination (MixDst): no ADD, no dense output.
// psgd_aggregate_mixed_ipc / psgd_aggregate_mixed_ipc_dst: the same two forms over the plan's IPC
// exchange session (psgd_aggregate_ipc on the residual between the ADD and the GATHER). Admission is
// the communicator forms' (the output pass takes the same route); the flat tail needs no staging:
// it is packed into the exchange slot and the last exchange stores its sums as bf16 (k_xchg_mix).
#include <memory>
#include <string>

#include "psgd_plan.h"

namespace {

// rank buckets 1 / 2 / 4 (VALU tiles) and 16 / 32 (matrix-core tiles, psgd_mixed_mfma.hip), fp32,
// not wide, one bucket. Rank bucket 8 (the VALU tile whose register-cached two-set instances sit at
// the scratch edge) and wide plans (ranks 33-128) have no mixed instance
const char* ineligible(const psgd_plan* p) {
    if (p->dtype != PSGD_F32) return "psgd_aggregate_mixed takes an fp32 plan (the fp32 residual of bf16 gradients)";
    const int rb = p->rbucket;
    if (p->wide() || !(rb == 1 || rb == 2 || rb == 4 || rb == 16 || rb == 32))
        return "psgd_aggregate_mixed serves rank buckets 1, 2, 4, 16 and 32 (not 8, not ranks above 32)";
    if (p->spans.size() > 1) return "psgd_aggregate_mixed takes a plan of one bucket";
    return nullptr;
}

// the context psgd_aggregate_mixed runs its step under (aggregate_ctx)
StepCtx mixed_ctx(const MixArgs* x, bool ingest) {
    StepCtx c;
    c.mix = x;
    c.mix_in = ingest;
    return world1_ctx(c);
}

// Admission: the runtime keeps at least two waves per SIMD of the instance a route's final pass
// would launch, without scratch (asked through the launch functions the drivers use)
bool admitted(hipError_t e, int waves) { return e == hipSuccess && waves >= 2; }
bool admitted(const psgd_plan* p, const IterRoute& r, const MixArgs& none) {
    int w = 0;
    return admitted(launch_final_pass(p, r, FinalArgs{}, &none, 0, nullptr, &w), w);
}
bool admitted(const psgd_plan* p, const OutRoute& o, const MixArgs& none, const MixDst* dst = nullptr) {
    int w = 0;
    ApplyArgs aa{};
    return admitted(launch_out_pass(p, o, aa, &none, 0, nullptr, &w, dst), w);
}

// (Re-)ask the runtime about the mixed instances this plan's current tiling would launch: per
// step parity its final pass, and its first pass where that is the single-pass ingest instance.
// The key covers every plan field the routes read that can change after creation (a re-tiling:
// fin_ok, fin_proj, oe_ok, fin_smax, out_nt); rank bucket, iterations and the knobs are fixed
void admit(psgd_plan* p) {
    psgd_plan::Mixed& m = *p->mixed;
    const uint64_t key = uint64_t(p->fin_ok) | uint64_t(p->fin_proj) << 1 | uint64_t(p->oe_ok) << 2 |
                         uint64_t(uint32_t(p->fin_smax)) << 8 | uint64_t(uint32_t(p->out_nt)) << 40;
    if (m.key == key) return;
    m.key = key;
    const MixArgs none{};
    m.fin_in = false;
    for (int par = 0; par < 2; ++par) {
        const IterRoute first = p->route(par, 0, mixed_ctx(&none, p->mix_ingest_on));
        if (first.pass == IterRoute::PassFinal && first.ingest) m.fin_in = admitted(p, first, none);
        const StepCtx c = mixed_ctx(&none, false);
        const IterRoute last = p->route(par, p->iters - 1, c);
        m.out[par] = last.pass == IterRoute::PassFinal ? admitted(p, last, none) : admitted(p, p->out_route(par, 1, c), none);
    }
}

// psgd_aggregate_mixed_comm: the bf16-output instance of the output pass, per communicator kind
// ([0]: world size > 1, [1]: a 1-rank communicator) and step parity. Its routes read fin_ok and
// out_nt of what a re-tiling can change: the key
void admit_comm(psgd_plan* p) {
    psgd_plan::Mixed& m = *p->mixed;
    const uint64_t key = uint64_t(p->fin_ok) | uint64_t(uint32_t(p->out_nt)) << 8;
    if (m.comm_key == key) return;
    m.comm_key = key;
    const MixArgs none{};
    for (int one = 0; one < 2; ++one)
        for (int par = 0; par < 2; ++par)
            m.comm_out[one][par] = admitted(p, p->out_route(par, one ? 1 : 2, comm_out_ctx(&none)), none);
}

bool comm_eligible(const psgd_plan* p, int world) {
    const psgd_plan::Mixed& m = *p->mixed;
    const int one = world == 1 ? 1 : 0;
    return m.comm_out[one][0] && m.comm_out[one][1];
}

// psgd_aggregate_mixed_comm_dst: the destination-table instance of the same output pass, asked
// for itself (its 2-byte store form is code the dense instance does not have); the routes read
// what admit_comm's read, under a key of its own
void admit_dst(psgd_plan* p) {
    psgd_plan::Mixed& m = *p->mixed;
    const uint64_t key = uint64_t(p->fin_ok) | uint64_t(uint32_t(p->out_nt)) << 8;
    if (m.dst_key == key) return;
    m.dst_key = key;
    const MixArgs none{};
    const MixDst tabs{};
    for (int one = 0; one < 2; ++one)
        for (int par = 0; par < 2; ++par)
            m.dst_out[one][par] = admitted(p, p->out_route(par, one ? 1 : 2, comm_out_ctx(&none, &tabs)), none, &tabs);
}

bool dst_eligible(const psgd_plan* p, int world) {
    const psgd_plan::Mixed& m = *p->mixed;
    const int one = world == 1 ? 1 : 0;
    return m.dst_out[one][0] && m.dst_out[one][1];
}

// The plan's mixed state: the bf16 gradients' pointer tables and the run-table ADD, device side in
// one allocation of the plan's own (made once, by the first call on a bound plan)
int ensure(psgd_plan* p) {
    if (p->mixed) return PSGD_OK;
    std::unique_ptr<psgd_plan::Mixed> m(new psgd_plan::Mixed());
    const size_t nt = p->shapes.size();
    std::vector<int64_t> zero(nt, 0), numel(nt, 1);
    std::vector<int32_t> idx(nt);
    for (size_t i = 0; i < nt; ++i) {
        idx[i] = int32_t(i);
        for (int64_t x : p->shapes[i]) numel[i] *= x;
    }
    p->mixed = m.release();
    psgd_plan::Mixed& mx = *p->mixed;
    if (int st = psgd_runs_create_mixed(zero.data(), idx.data(), zero.data(), numel.data(), idx.data(), int32_t(nt),
                                        int32_t(nt), int32_t(nt), PSGD_BF16, PSGD_F32, &mx.add))
        return st;
    int64_t rb = 0;
    if (int st = psgd_runs_workspace_bytes(mx.add, &rb)) return st;
    const size_t tab = align256(TableCache::bytes(nt));  // src_tab, then dst, then the ADD's workspace
    PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&mx.dev), 2 * tab + size_t(rb)));
    mx.add_ws = mx.dev + 2 * tab;
    mx.src_tab.bind(mx.dev, nt);
    mx.dst.bind(mx.dev + tab, nt);
    return psgd_runs_bind(mx.add, p->device, mx.add_ws);
}

void folds_at(const psgd_plan* p, int64_t step, int32_t* in, int32_t* out) {
    const psgd_plan::Mixed& m = *p->mixed;
    const bool eligible = m.out[0] && m.out[1];
    // the step's only gradient pass is the single-pass final kernel
    const IterRoute first = p->route(step, 0, mixed_ctx(nullptr, true));
    const bool single = first.pass == IterRoute::PassFinal && first.ingest;
    *out = eligible ? 1 : 0;
    *in = eligible && single && m.fin_in ? 1 : 0;
}

// room for the uncompressed bf16 gradients' pointer table and, behind it, their destinations'
// (first call, or a larger flat plan than the last one's), and the null checks of both tensor
// lists (`unc`: the bf16 gradients, or the bf16 destinations of psgd_aggregate_mixed_comm_dst)
int unc_table(psgd_plan::Mixed& m, psgd_flat* f, void* const* unc, void* const* unc_residual, hipStream_t s) {
    const size_t cnt = size_t(f->count);
    if (cnt > m.unc_cap) {
        PSGD_HIP(hipStreamSynchronize(s));
        m.unc_tab.release();
        m.unc_dst.release();
        if (m.unc_dev) PSGD_HIP(hipFree(m.unc_dev));
        m.unc_dev = nullptr;
        m.unc_cap = 0;
        PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&m.unc_dev), 2 * TableCache::bytes(cnt)));
        m.unc_cap = cnt;
        m.unc_tab.bind(m.unc_dev, cnt);
        m.unc_dst.bind(m.unc_dev + TableCache::bytes(cnt), cnt);
    } else if (m.unc_tab.n != cnt) {
        PSGD_HIP(hipStreamSynchronize(s));
        m.unc_tab.bind(m.unc_dev, cnt);
        m.unc_dst.bind(m.unc_dev + TableCache::bytes(cnt), cnt);
    }
    for (int32_t i = 0; i < f->count; ++i)
        if (!unc[i] || !unc_residual[i]) return fail(PSGD_ERR_VALUE, "null uncompressed tensor pointer");
    return PSGD_OK;
}

// the plan's eligibility, then every tensor's two pointers
int check_tensors(const psgd_plan* p, void* const* grads, void* const* residual) {
    if (const char* why = ineligible(p)) return fail(PSGD_ERR_VALUE, why);
    for (size_t i = 0; i < p->shapes.size(); ++i) {
        if (!grads[i] || !residual[i]) return fail(PSGD_ERR_VALUE, "null gradient pointer");
        if (reinterpret_cast<uintptr_t>(grads[i]) % 2) return fail(PSGD_ERR_LAYOUT, "bf16 gradients must be 2-byte aligned");
        if (reinterpret_cast<uintptr_t>(residual[i]) % 4) return fail(PSGD_ERR_LAYOUT, "the fp32 residual must be 4-byte aligned");
    }
    return PSGD_OK;
}

// A fold query: admission is a property of this build's kernels on the device (asked once per
// tiling); the query caches it in the plan like the first mixed call does. A plan with no device
// yet asks without keeping device state (a temporary Mixed for the duration of the query).
template <typename Read>
int query_folds(const psgd_plan* plan, void (*admit_fn)(psgd_plan*), Read read) {
    psgd_plan* p = const_cast<psgd_plan*>(plan);
    DevScope scope(p->device);
    psgd_plan::Mixed tmp;
    const bool unbound = !p->mixed && !p->bound;
    if (unbound) p->mixed = &tmp;
    if (!p->mixed)
        if (int st = ensure(p)) return st;
    admit_fn(p);
    read(p);
    if (unbound) p->mixed = nullptr;
    return PSGD_OK;
}

int mixed_impl(psgd_plan* p, void* const* grads, void* const* residual, void* out, int64_t step, psgd_flat* f,
               void* const* unc, void* const* unc_residual, void* flat_out, hipStream_t s) {
    if (int st = check_tensors(p, grads, residual)) return st;
    DevScope scope(p->device);
    if (int st = ensure(p)) return st;
    psgd_plan::Mixed& m = *p->mixed;
    // the tiling the step will run on (the residual's alignment decides the vector layout)
    if (int st = refresh_pointers(p, residual, s)) return st;
    admit(p);
    int32_t in = 0, fo = 0;
    folds_at(p, step, &in, &fo);
    if (!fo)
        return fail(PSGD_ERR_VALUE, "psgd_aggregate_mixed: no admitted bf16-output instance of this plan's final pass "
                                    "(two waves per SIMD, no scratch)");
    FlatArgs fa{};
    MixArgs x{};
    if (f) {
        if (int st = unc_table(m, f, unc, unc_residual, s)) return st;
        if (int st = flat_args(f, unc_residual, flat_out, 1, s, &fa)) return st;
        PSGD_HIP(m.unc_tab.select(unc, s));
        x.unc_src = m.unc_tab.table();
    }
    if (in) {
        PSGD_HIP(m.src_tab.select(grads, s));
        x.src = m.src_tab.table();
    } else {
        if (int st = psgd_runs_add_list(m.add, grads, residual, 1, s)) return st;
    }
    StepCtx c = mixed_ctx(&x, in != 0);
    c.fl = f ? &fa : nullptr;
    c.out = out;
    return aggregate_ctx(p, residual, step, s, c);
}

// the fp32 staging of the flat tail (first call, or a larger flat plan than the last one's)
int stage_room(psgd_plan::Mixed& m, const psgd_flat* f, hipStream_t s) {
    if (size_t(f->total) <= m.stage_cap) return PSGD_OK;
    PSGD_HIP(hipStreamSynchronize(s));
    if (m.stage) PSGD_HIP(hipFree(m.stage));
    m.stage = nullptr;
    m.stage_cap = 0;
    PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&m.stage), size_t(f->total) * sizeof(float)));
    m.stage_cap = size_t(f->total);
    return PSGD_OK;
}

// psgd_aggregate_mixed_comm past its argument checks. *refused: the plan has no admitted instance
// (nothing launched, no collective issued: the communicator stays usable)
int mixed_comm_impl(psgd_plan* p, void* const* grads, void* const* residual, void* out, int64_t step, psgd_flat* f,
                    void* const* unc, void* const* unc_residual, void* flat_out, psgd_comm* comm, hipStream_t s,
                    bool* refused) {
    DevScope scope(p->device);
    if (int st = ensure(p)) return st;
    psgd_plan::Mixed& m = *p->mixed;
    // the tiling the step will run on (the residual's alignment decides the vector layout)
    if (int st = refresh_pointers(p, residual, s)) return st;
    admit_comm(p);
    if (!comm_eligible(p, comm_world(comm))) {
        *refused = true;
        return fail(PSGD_ERR_VALUE, "psgd_aggregate_mixed_comm: no admitted bf16-output instance of this plan's final "
                                    "pass (two waves per SIMD, no scratch)");
    }
    MixArgs x{};
    if (f) {
        if (int st = unc_table(m, f, unc, unc_residual, s)) return st;
        if (int st = stage_room(m, f, s)) return st;
        PSGD_HIP(m.unc_tab.select(unc, s));
        x.unc_src = m.unc_tab.table();
        x.stage = m.stage;
    }
    if (int st = psgd_runs_add_list(m.add, grads, residual, 1, s)) return st;
    return aggregate_comm_ctx(p, residual, out, step, f, unc_residual, flat_out, comm, s, &x);
}

// psgd_aggregate_mixed_comm_dst past its argument checks (`refused` as in mixed_comm_impl)
int mixed_dst_impl(psgd_plan* p, void* const* residual, void* const* dst, int64_t step, psgd_flat* f,
                   void* const* unc_residual, void* const* unc_dst, psgd_comm* comm, hipStream_t s, bool* refused) {
    DevScope scope(p->device);
    if (int st = ensure(p)) return st;
    psgd_plan::Mixed& m = *p->mixed;
    // the tiling the step will run on: the residual's alignment decides the vector layout, as in
    // the three-stage flow; the destinations' alignment only picks the store form, in the kernel
    if (int st = refresh_pointers(p, residual, s)) return st;
    admit_dst(p);
    if (!dst_eligible(p, comm_world(comm))) {
        *refused = true;
        return fail(PSGD_ERR_VALUE, "psgd_aggregate_mixed_comm_dst: no admitted destination-table instance of this "
                                    "plan's final pass (two waves per SIMD, no scratch)");
    }
    MixArgs x{};
    MixDst t{};
    if (f) {
        if (int st = unc_table(m, f, unc_dst, unc_residual, s)) return st;
        if (int st = stage_room(m, f, s)) return st;
        PSGD_HIP(m.unc_dst.select(unc_dst, s));
        t.unc_dst = m.unc_dst.table();
        x.stage = m.stage;
    }
    PSGD_HIP(m.dst.select(dst, s));
    t.dst = m.dst.table();
    return aggregate_comm_ctx(p, residual, nullptr, step, f, unc_residual, nullptr, comm, s, &x, &t);
}

// psgd_aggregate_mixed_ipc / psgd_aggregate_mixed_ipc_dst past their argument checks: the
// session's state, then admission for the session's world size (the output pass of the IPC step
// takes the communicator step's route: the same instances, the same admission), then the pointer
// tables. Everything that can refuse comes before the ADD. No staging buffer: the flat tail lives
// in the exchange slot and k_xchg_mix stores its sums as bf16
int mixed_ipc_impl(psgd_plan* p, void* const* grads, void* const* residual, void* out, int64_t step, psgd_flat* f,
                   void* const* unc, void* const* unc_residual, void* flat_out, hipStream_t s) {
    if (int st = ipc_check(p, step)) return st;
    if (f && f->total > p->ipc_flat_cap)
        return fail(PSGD_ERR_VALUE, "flat tensors exceed the exchange buffer (psgd_ipc_create)");
    DevScope scope(p->device);
    if (int st = ensure(p)) return st;
    psgd_plan::Mixed& m = *p->mixed;
    // the tiling the step will run on (the residual's alignment decides the vector layout)
    if (int st = refresh_pointers(p, residual, s)) return st;
    admit_comm(p);
    if (!comm_eligible(p, p->ipc_world))
        return fail(PSGD_ERR_VALUE, "psgd_aggregate_mixed_ipc: no admitted bf16-output instance of this plan's final "
                                    "pass (two waves per SIMD, no scratch)");
    MixArgs x{};
    if (f) {
        if (int st = unc_table(m, f, unc, unc_residual, s)) return st;
        PSGD_HIP(m.unc_tab.select(unc, s));
        x.unc_src = m.unc_tab.table();
    }
    if (int st = psgd_runs_add_list(m.add, grads, residual, 1, s)) return st;
    return aggregate_ipc_ctx(p, residual, out, step, f, unc_residual, flat_out, s, &x, nullptr);
}

int mixed_ipc_dst_impl(psgd_plan* p, void* const* residual, void* const* dst, int64_t step, psgd_flat* f,
                       void* const* unc_residual, void* const* unc_dst, hipStream_t s) {
    if (int st = ipc_check(p, step)) return st;
    if (f && f->total > p->ipc_flat_cap)
        return fail(PSGD_ERR_VALUE, "flat tensors exceed the exchange buffer (psgd_ipc_create)");
    DevScope scope(p->device);
    if (int st = ensure(p)) return st;
    psgd_plan::Mixed& m = *p->mixed;
    if (int st = refresh_pointers(p, residual, s)) return st;
    admit_dst(p);
    if (!dst_eligible(p, p->ipc_world))
        return fail(PSGD_ERR_VALUE, "psgd_aggregate_mixed_ipc_dst: no admitted destination-table instance of this "
                                    "plan's final pass (two waves per SIMD, no scratch)");
    MixArgs x{};
    MixDst t{};
    if (f) {
        if (int st = unc_table(m, f, unc_dst, unc_residual, s)) return st;
        PSGD_HIP(m.unc_dst.select(unc_dst, s));
        t.unc_dst = m.unc_dst.table();
    }
    PSGD_HIP(m.dst.select(dst, s));
    t.dst = m.dst.table();
    return aggregate_ipc_ctx(p, residual, nullptr, step, f, unc_residual, nullptr, s, &x, &t);
}

}  // namespace

void psgd::mixed_release(psgd_plan* p) {
    if (!p->mixed) return;
    psgd_plan::Mixed* m = p->mixed;
    m->src_tab.release();
    m->unc_tab.release();
    m->dst.release();
    m->unc_dst.release();
    if (m->add) (void)psgd_runs_destroy(m->add);
    if (m->dev) (void)hipFree(m->dev);
    if (m->unc_dev) (void)hipFree(m->unc_dev);
    if (m->stage) (void)hipFree(m->stage);
    delete m;
    p->mixed = nullptr;
}

extern "C" {

int psgd_plan_mixed_folds(const psgd_plan* plan, int64_t step, int32_t* fold_in, int32_t* fold_out) {
    if (!plan || !fold_in || !fold_out) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    *fold_in = *fold_out = 0;
    if (ineligible(plan)) return PSGD_OK;
    return query_folds(plan, admit, [&](const psgd_plan* p) { folds_at(p, step, fold_in, fold_out); });
}

int psgd_aggregate_mixed_flat(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16, int64_t step,
                              psgd_flat* f, void* const* unc_bf16, void* const* unc_residual, void* flat_out_bf16,
                              void* stream) {
    if (int st = check_call(p && grads_bf16 && residual && out_bf16, p && p->bound, step >= 0, "step out of range"))
        return st;
    if (int st = check_out(out_bf16)) return st;
    const bool has_flat = f && f->total > 0;
    if (has_flat)
        if (int st = check_flat(f, unc_bf16 && unc_residual && flat_out_bf16, f->dtype == PSGD_F32 && f->device == p->device,
                                PSGD_ERR_VALUE, "psgd_aggregate_mixed_flat takes an fp32 flat plan (the uncompressed tensors' "
                                                "residual) on the codec's device"))
            return st;
    return mixed_impl(p, grads_bf16, residual, out_bf16, step, has_flat ? f : nullptr, unc_bf16, unc_residual,
                      flat_out_bf16, static_cast<hipStream_t>(stream));
}

int psgd_plan_mixed_folds_comm(const psgd_plan* plan, int64_t step, int32_t world, int32_t* fold_in,
                               int32_t* fold_out) {
    if (!plan || !fold_in || !fold_out) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (world < 1) return fail(PSGD_ERR_VALUE, "world size must be >= 1");
    *fold_in = *fold_out = 0;  // no ingest fold in this form: the ADD is always a launch of its own
    if (ineligible(plan)) return PSGD_OK;
    return query_folds(plan, admit_comm, [&](const psgd_plan* p) { *fold_out = comm_eligible(p, world) ? 1 : 0; });
}

int psgd_aggregate_mixed_comm(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16,
                              int64_t step, psgd_flat* f, void* const* unc_bf16, void* const* unc_residual,
                              void* flat_out_bf16, psgd_comm* comm, void* stream) {
    if (int st = check_call(p && grads_bf16 && residual && out_bf16 && comm, p && p->bound, step >= 0, "step out of range"))
        return st;
    if (int st = check_out(out_bf16)) return st;
    const bool has_flat = f && f->total > 0;
    if (has_flat)
        if (int st = check_flat(f, unc_bf16 && unc_residual && flat_out_bf16, f->dtype == PSGD_F32 && f->device == p->device,
                                PSGD_ERR_VALUE, "psgd_aggregate_mixed_comm takes an fp32 flat plan (the uncompressed tensors' "
                                                "residual) on the codec's device"))
            return st;
    if (int st = check_tensors(p, grads_bf16, residual)) return st;
    // a poisoned communicator is refused before the step launches anything: the caller's
    // gradients, the residual and the P/Q state stay as they were
    std::string why;
    if (comm_poisoned(comm, &why))
        return fail(PSGD_ERR_STATE, ("communicator unusable after an earlier failure: " + why).c_str());
    bool refused = false;
    const int st = mixed_comm_impl(p, grads_bf16, residual, out_bf16, step, has_flat ? f : nullptr, unc_bf16,
                                   unc_residual, flat_out_bf16, comm, static_cast<hipStream_t>(stream), &refused);
    // a failure past the argument checks can leave this rank's collective sequence short of its
    // peers': the communicator refuses every later call (psgd_comm.cpp, comm_poison)
    if (st && !refused) comm_poison(comm, psgd_last_error());
    return st;
}

int psgd_plan_mixed_folds_dst(const psgd_plan* plan, int64_t step, int32_t world, int32_t* fold_out) {
    if (!plan || !fold_out) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (world < 1) return fail(PSGD_ERR_VALUE, "world size must be >= 1");
    *fold_out = 0;
    if (ineligible(plan)) return PSGD_OK;
    return query_folds(plan, admit_dst, [&](const psgd_plan* p) { *fold_out = dst_eligible(p, world) ? 1 : 0; });
}

int psgd_aggregate_mixed_comm_dst(psgd_plan* p, void* const* residual, void* const* dst_bf16, int64_t step,
                                  psgd_flat* f, void* const* unc_residual, void* const* unc_dst_bf16, psgd_comm* comm,
                                  void* stream) {
    if (int st = check_call(p && residual && dst_bf16 && comm, p && p->bound, step >= 0, "step out of range")) return st;
    const bool has_flat = f && f->total > 0;
    if (has_flat)
        if (int st = check_flat(f, unc_residual && unc_dst_bf16, f->dtype == PSGD_F32 && f->device == p->device,
                                PSGD_ERR_VALUE, "psgd_aggregate_mixed_comm_dst takes an fp32 flat plan (the uncompressed "
                                                "tensors' residual) on the codec's device"))
            return st;
    // eligibility, then every tensor's two pointers: the destinations are bf16 like the gradients
    if (int st = check_tensors(p, dst_bf16, residual)) return st;
    std::string why;
    if (comm_poisoned(comm, &why))
        return fail(PSGD_ERR_STATE, ("communicator unusable after an earlier failure: " + why).c_str());
    bool refused = false;
    const int st = mixed_dst_impl(p, residual, dst_bf16, step, has_flat ? f : nullptr, unc_residual, unc_dst_bf16, comm,
                                  static_cast<hipStream_t>(stream), &refused);
    if (st && !refused) comm_poison(comm, psgd_last_error());
    return st;
}

int psgd_aggregate_mixed_ipc(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16, int64_t step,
                             psgd_flat* f, void* const* unc_bf16, void* const* unc_residual, void* flat_out_bf16,
                             void* stream) {
    // the argument errors (null, a negative step) before the plan's state
    if (!p || !grads_bf16 || !residual || !out_bf16) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (int st = check_out(out_bf16)) return st;
    const bool has_flat = f && f->total > 0;
    if (has_flat)
        if (int st = check_flat(f, unc_bf16 && unc_residual && flat_out_bf16, f->dtype == PSGD_F32 && f->device == p->device,
                                PSGD_ERR_VALUE, "psgd_aggregate_mixed_ipc takes an fp32 flat plan (the uncompressed tensors' "
                                                "residual) on the codec's device"))
            return st;
    if (int st = check_tensors(p, grads_bf16, residual)) return st;
    return mixed_ipc_impl(p, grads_bf16, residual, out_bf16, step, has_flat ? f : nullptr, unc_bf16, unc_residual,
                          flat_out_bf16, static_cast<hipStream_t>(stream));
}

int psgd_aggregate_mixed_ipc_dst(psgd_plan* p, void* const* residual, void* const* dst_bf16, int64_t step, psgd_flat* f,
                                 void* const* unc_residual, void* const* unc_dst_bf16, void* stream) {
    if (!p || !residual || !dst_bf16) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    const bool has_flat = f && f->total > 0;
    if (has_flat)
        if (int st = check_flat(f, unc_residual && unc_dst_bf16, f->dtype == PSGD_F32 && f->device == p->device,
                                PSGD_ERR_VALUE, "psgd_aggregate_mixed_ipc_dst takes an fp32 flat plan (the uncompressed "
                                                "tensors' residual) on the codec's device"))
            return st;
    // eligibility, then every tensor's two pointers: the destinations are bf16 like the gradients
    if (int st = check_tensors(p, dst_bf16, residual)) return st;
    return mixed_ipc_dst_impl(p, residual, dst_bf16, step, has_flat ? f : nullptr, unc_residual, unc_dst_bf16,
                              static_cast<hipStream_t>(stream));
}

int psgd_aggregate_mixed(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16, int64_t step,
                         void* stream) {
    return psgd_aggregate_mixed_flat(p, grads_bf16, residual, out_bf16, step, nullptr, nullptr, nullptr, nullptr,
                                     stream);
}

}  // extern "C"
