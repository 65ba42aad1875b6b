// The one-call steps that store their averages through an OutSink (psgd_plan.h), and their queries
// (include/psgd.h). Each is DEFINED as a sequence of the plain calls and equal to it bit for bit:
//   bf16 sinks   the fp32 codec on an fp32 error-feedback residual fed by bf16 gradients:
//                  residual += float(g); g = +0.0   (psgd_runs_add_list, zero_source: "the ADD")
//                  psgd_aggregate[_flat] / psgd_aggregate_comm / psgd_aggregate_ipc on the residual
//                  out = bf16(averages)             (psgd_runs_gather)
//                psgd_aggregate_mixed[_flat] at world size 1, _comm over a communicator, _ipc over
//                the plan's exchange session, _wide[_comm] on a wide plan (ranks 33-128). The ADD is
//                the first launch, but on the steps of psgd_aggregate_mixed whose only gradient pass
//                is the single-pass k_final_odd (I = 1, odd step, ranks 1 / 2), which ingests there.
//                _comm_dst / _ipc_dst: the DDP hook's form. The residual already holds residual +
//                gradients (the hook adds each bucket on arrival): no ADD, and the final pass stores
//                each tensor's bf16 average at the tensor's own destination.
//   fp32 tables  psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst, the default DDP hook's completion:
//                psgd_aggregate_comm (psgd_aggregate_ipc) on the gradients with every fp32 average
//                stored at the tensor's own destination, so no slab is written and no gather runs.
//   fp32 update  psgd_aggregate_comm_sgd: psgd_aggregate_comm_dst into scratch destinations, then
//                psgd_sgd_update on them; the final pass applies the SGD update to the weights and the
//                momentum buffers at the element where it would have stored the average.
//   fp32 adam    psgd_aggregate_comm_adam: the same with psgd_adam_update (torch's Adam / AdamW rule on
//                the weights and both moments).
//   bf16 master  psgd_aggregate_mixed_comm_adam: the ADD, psgd_aggregate_comm_dst on the residual into
//                scratch destinations, psgd_adam_update_mp on them: the final pass updates the fp32
//                master weights and moments and stores bf16(p') at the model parameters.
//   wide adam    psgd_aggregate_comm_adam_wide / psgd_aggregate_mixed_comm_adam_wide (ranks 33-128): the two
//                above with psgd_aggregate_comm's slabs in place of the scratch destinations (a wide plan
//                has no destination-table step); the final pass is k_wide_apply_adam.
//   wide sgd     psgd_aggregate_comm_sgd_wide (ranks 33-128): psgd_aggregate_comm into scratch slabs, then
//                psgd_sgd_update on them; the final pass is k_wide_apply_sgd.
//   sgd master   psgd_aggregate_mixed_comm_sgd (and _wide on ranks 33-128): the ADD, then the fp32 update
//                entry's sequence with psgd_sgd_update_mp: the final pass (k_apply_sgd_mp / k_lowrank_sgd_mp;
//                k_wide_apply_sgd_mp) updates the fp32 master weights and momentum buffers and stores
//                bf16(p') at the model parameters.
//   wide tables  psgd_aggregate_comm_dst_wide / psgd_aggregate_mixed_comm_dst_wide (ranks 33-128), the DDP
//                hook's completions on a wide plan: psgd_aggregate_comm into scratch slabs, then every
//                average copied (bf16: rounded) to the tensor's own destination; the final pass is
//                k_wide_apply_dst, which stores there and writes no slab.
// Every entry is a descriptor (Entry) and its arguments (Call): one preamble runs the checks in the
// entry's documented order, one body makes the side state, asks admission (a refusal launches
// nothing), builds the sink and hands it to the step driver of the entry's transport.
#include <string>

#include "psgd_plan.h"

namespace {

using Adm = psgd_plan::Admission;

struct Entry {
    const char* name;  // for messages
    enum Via { World1, Comm, Xchg } via;
    bool wide, tables, bf16;
    bool sgd = false;  // the update sink: `peer` the parameters, Call::bufs / hyper beside them; a null
                       // communicator is world size 1 without collectives
    bool adam = false;  // the Adam update sink: Call::bufs / vs the two moments, Call::adam the records
    bool mp = false;  // adam or sgd over fp32 master weights of a bf16 model: `state` the residual, `peer`
                      // the masters, Call::grads16 / ws the bf16 gradients and model parameters
    bool upd() const { return sgd || adam; }
    bool wide_dst() const { return wide && tables && !upd(); }  // the wide destination-table entries
    Adm::Kind kind() const {
        if (wide_dst()) return bf16 ? Adm::Bf16TablesWide : Adm::F32TablesWide;
        if (adam && wide) return mp ? Adm::F32AdamMpWide : Adm::F32AdamWide;
        if (sgd && wide) return mp ? Adm::F32SgdMpWide : Adm::F32SgdWide;
        if (sgd && mp) return Adm::F32SgdMp;
        return mp ? Adm::F32AdamMp : adam ? Adm::F32Adam : sgd ? Adm::F32Sgd : !bf16 ? Adm::F32Tables : tables ? Adm::Bf16Tables : Adm::Bf16Dense;
    }
};

// The arguments by role. `state`: the fp32 tensors the codec runs on (a bf16 sink: the residual; else
// the gradients); `peer`: per tensor the bf16 gradient (dense sinks) or the destination (tables).
// `unc_state` / `unc_peer`: the same of the flat plan's tensors. `out` / `flat_out`: dense sinks.
struct Call {
    psgd_plan* p;
    void* const* state;
    void* const* peer;
    void* out;
    int64_t step;
    psgd_flat* f;
    void* const* unc_state;
    void* const* unc_peer;
    void* flat_out;
    psgd_comm* comm;
    void* stream;
    // the update sink: momentum buffers (a table or an entry may be null where momentum == 0) and
    // the records, the plan's tensors first
    void* const* bufs = nullptr;
    void* const* unc_bufs = nullptr;
    const psgd_sgd_hyper* hyper = nullptr;
    // the Adam sink: `bufs` / `unc_bufs` the first moments, these the second, and its records
    void* const* vs = nullptr;
    void* const* unc_vs = nullptr;
    const psgd_adam_hyper* adam = nullptr;
    // the master-weight sink: the bf16 gradients the ADD consumes and the bf16 model parameters
    void* const* grads16 = nullptr;
    void* const* unc_grads16 = nullptr;
    void* const* ws = nullptr;
    void* const* unc_ws = nullptr;
};

// The plans an entry serves, by shape. bf16 sinks: fp32, one bucket, rank buckets 1 / 2 / 4 (VALU
// tiles) and 16 / 32 (matrix-core tiles, psgd_mixed_mfma.hip), not 8 (the VALU tile whose
// register-cached two-set instances sit at the scratch edge); the wide entries: what those refuse by
// rank. fp32 tables: fp32, one bucket, not wide
const char* ineligible(const psgd_plan* p, bool bf16, bool wide, int* code, bool sgd = false, bool adam = false,
                       bool wide_dst = false) {
    *code = PSGD_ERR_VALUE;
    const int rb = p->rbucket;
    if (wide_dst && !bf16) {  // the wide destination-table entries: what the narrow ones refuse by rank
        if (p->dtype != PSGD_F32) {
            *code = PSGD_ERR_DTYPE;
            return "psgd_aggregate_comm_dst_wide takes an fp32 plan";
        }
        if (!p->wide()) return "psgd_aggregate_comm_dst_wide serves ranks 33-128 (psgd_aggregate_comm_dst: rank buckets 1 to 32)";
        if (p->spans.size() > 1) return "psgd_aggregate_comm_dst_wide takes a plan of one bucket";
    } else if (wide_dst) {
        if (p->dtype != PSGD_F32)
            return "psgd_aggregate_mixed_comm_dst_wide takes an fp32 plan (the fp32 residual of bf16 gradients)";
        if (!p->wide())
            return "psgd_aggregate_mixed_comm_dst_wide serves ranks 33-128 (psgd_aggregate_mixed_comm_dst: rank buckets 1, "
                   "2, 4, 16 and 32)";
        if (p->spans.size() > 1) return "psgd_aggregate_mixed_comm_dst_wide takes a plan of one bucket";
    } else if (adam && wide) {  // the wide Adam entries: what the narrow ones refuse by rank
        if (p->dtype != PSGD_F32) {
            *code = PSGD_ERR_DTYPE;
            return "psgd_aggregate_comm_adam_wide takes an fp32 plan";
        }
        if (!p->wide()) return "psgd_aggregate_comm_adam_wide serves ranks 33-128 (psgd_aggregate_comm_adam: rank buckets 1 to 32)";
        if (p->spans.size() > 1) return "psgd_aggregate_comm_adam_wide takes a plan of one bucket";
    } else if (adam) {
        if (p->dtype != PSGD_F32) {
            *code = PSGD_ERR_DTYPE;
            return "psgd_aggregate_comm_adam takes an fp32 plan";
        }
        if (p->wide()) return "psgd_aggregate_comm_adam serves rank buckets 1 to 32";
        if (p->spans.size() > 1) return "psgd_aggregate_comm_adam takes a plan of one bucket";
    } else if (sgd && wide) {  // the wide SGD entry: what the narrow one refuses by rank
        if (p->dtype != PSGD_F32) {
            *code = PSGD_ERR_DTYPE;
            return "psgd_aggregate_comm_sgd_wide takes an fp32 plan";
        }
        if (!p->wide()) return "psgd_aggregate_comm_sgd_wide serves ranks 33-128 (psgd_aggregate_comm_sgd: rank buckets 1 to 32)";
        if (p->spans.size() > 1) return "psgd_aggregate_comm_sgd_wide takes a plan of one bucket";
    } else if (sgd) {
        if (p->dtype != PSGD_F32) {
            *code = PSGD_ERR_DTYPE;
            return "psgd_aggregate_comm_sgd takes an fp32 plan";
        }
        if (p->wide()) return "psgd_aggregate_comm_sgd serves rank buckets 1 to 32";
        if (p->spans.size() > 1) return "psgd_aggregate_comm_sgd takes a plan of one bucket";
    } else if (!bf16) {
        if (p->dtype != PSGD_F32) {
            *code = PSGD_ERR_DTYPE;
            return "psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst take an fp32 plan";
        }
        if (p->wide()) return "psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst serve rank buckets 1 to 32";
        if (p->spans.size() > 1) return "psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst take a plan of one bucket";
    } else if (wide) {
        if (p->dtype != PSGD_F32)
            return "psgd_aggregate_mixed_wide takes an fp32 plan (the fp32 residual of bf16 gradients)";
        if (!p->wide())
            return "psgd_aggregate_mixed_wide serves ranks 33-128 (psgd_aggregate_mixed: rank buckets 1, 2, 4, 16 and 32)";
        if (p->spans.size() > 1) return "psgd_aggregate_mixed_wide takes a plan of one bucket";
    } else {
        if (p->dtype != PSGD_F32) return "psgd_aggregate_mixed takes an fp32 plan (the fp32 residual of bf16 gradients)";
        if (p->wide() || !(rb == 1 || rb == 2 || rb == 4 || rb == 16 || rb == 32))
            return "psgd_aggregate_mixed serves rank buckets 1, 2, 4, 16 and 32 (not 8, not ranks above 32)";
        if (p->spans.size() > 1) return "psgd_aggregate_mixed takes a plan of one bucket";
    }
    return nullptr;
}

// ------------------------------------------------------------------ admission ------
// One cell: the instance the final pass of parity `par` would launch for a sink of `kind` under a
// communicator kind, asked with ntiles = 0 through the launch functions the drivers use. NoComm is
// aggregate_ctx's context (the fused final pass where the step has one); Bf16Ingest its single-pass
// final kernel with the ingest fold (false where the step's first pass is another one). A wide
// plan's sink instances are k_wide_apply_mix<rbucket>, k_wide_apply_adam<rbucket>,
// k_wide_apply_sgd[_mp]<rbucket> and k_wide_apply_dst<rbucket> (shared terms at world size 1)
bool ask(const psgd_plan* p, Adm::Kind kind, Adm::Comm comm, int par) {
    OutSink sink;
    sink.sgd = kind == Adm::F32Sgd || kind == Adm::F32SgdMp;
    sink.sgd_mp = kind == Adm::F32SgdMp;
    sink.adam = kind == Adm::F32Adam || kind == Adm::F32AdamMp;
    sink.adam_mp = kind == Adm::F32AdamMp;
    sink.bf16 = kind != Adm::F32Tables && !sink.sgd && !sink.adam;
    sink.tables = kind == Adm::Bf16Tables || kind == Adm::F32Tables || sink.sgd || sink.adam;
    const int world = comm == Adm::Many ? 2 : 1;
    int w = 0;
    hipError_t e = hipErrorInvalidValue;
    if (p->wide()) {
        WideArgs a{};
        a.shared = world == 1;
        if (kind == Adm::Bf16Dense) e = launch_wide_apply_mix(p->rbucket, a, 0, nullptr, &w);
        else if (kind == Adm::F32AdamWide || kind == Adm::F32AdamMpWide)
            e = launch_wide_apply_adam(p->rbucket, kind == Adm::F32AdamMpWide, a, WideAdamDst{}, 0, nullptr, &w);
        else if (kind == Adm::F32SgdWide)
            e = launch_wide_apply_sgd(p->rbucket, a, WideSgdDst{}, 0, nullptr, &w);
        else if (kind == Adm::F32SgdMpWide)
            e = launch_wide_apply_sgd_mp(p->rbucket, a, WideSgdMpDst{}, 0, nullptr, &w);
        else if (kind == Adm::F32TablesWide || kind == Adm::Bf16TablesWide)
            e = launch_wide_apply_dst(p->rbucket, kind == Adm::Bf16TablesWide, a, WideDst{}, 0, nullptr, &w);
    } else if (comm == Adm::NoComm) {
        StepCtx c = world1_ctx(out_ctx(&sink));
        c.mix_in = kind == Adm::Bf16Ingest && p->mix_ingest_on;
        const IterRoute r = p->route(par, kind == Adm::Bf16Ingest ? 0 : p->iters - 1, c);
        ApplyArgs aa{};
        if (r.pass == IterRoute::PassFinal && (kind != Adm::Bf16Ingest || r.ingest))
            e = launch_final_pass(p, r, FinalArgs{}, &sink, 0, nullptr, &w);
        else if (kind != Adm::Bf16Ingest)
            e = launch_out_pass(p, p->out_route(par, 1, c), aa, &sink, 0, nullptr, &w);
    } else {
        ApplyArgs aa{};
        e = launch_out_pass(p, p->out_route(par, world, out_ctx(&sink)), aa, &sink, 0, nullptr, &w);
    }
    return e == hipSuccess && w >= 2;
}

// Both parities of (kind, comm) are admitted on the plan's current tiling; asked once per key. The
// key covers every plan field the routes read that can change after creation (a re-tiling: fin_ok,
// fin_proj, oe_ok, fin_smax, out_nt); rank bucket, iterations and the knobs are fixed
bool admitted(psgd_plan* p, Adm::Kind kind, Adm::Comm comm) {
    Adm& a = p->adm;
    const uint64_t key = uint64_t(p->fin_ok) | uint64_t(p->fin_proj) << 1 | uint64_t(p->oe_ok) << 2 |
                         uint64_t(uint32_t(p->fin_smax)) << 8 | uint64_t(uint32_t(p->out_nt)) << 40;
    if (a.key != key) {
        a = Adm{};
        a.key = key;
    }
    if (!a.asked[kind][comm]) {
        a.asked[kind][comm] = true;
        for (int par = 0; par < 2; ++par) a.ok[kind][comm][par] = ask(p, kind, comm, par);
    }
    return a.ok[kind][comm][0] && a.ok[kind][comm][1];
}

// A communicator's world size is known only at the call: the bf16 sinks of the narrow plans answer
// per communicator kind; the wide entries and the fp32 tables are eligible as a whole plan or not
bool eligible(psgd_plan* p, const Entry& e, int world) {
    if (e.via == Entry::World1 && !e.wide) return admitted(p, e.kind(), Adm::NoComm);
    // a wide plan has no destination-table instances: its Adam entries are defined against
    // psgd_aggregate_comm's slab, and ask for k_wide_apply_adam of the communicator kind alone; its
    // destination-table entries likewise for k_wide_apply_dst. Its SGD entry serves the plans both
    // of whose forms (k_wide_apply_sgd with shared terms and with two term sets) are admitted
    if (e.wide && e.sgd) return admitted(p, e.kind(), Adm::One) && admitted(p, e.kind(), Adm::Many);
    if (e.wide && (e.adam || e.tables)) return admitted(p, e.kind(), world == 1 ? Adm::One : Adm::Many);
    // an update entry is defined as the destination-table step followed by psgd_sgd_update /
    // psgd_adam_update: it serves the plans whose destination instances are admitted too
    if (e.upd() && !(admitted(p, Adm::F32Tables, Adm::Many) && admitted(p, Adm::F32Tables, Adm::One))) return false;
    // a master-weight entry applies psgd_plan_adam_ok's / psgd_plan_sgd_ok's rule, then asks for its
    // own instances
    const Adm::Kind base = e.adam ? Adm::F32Adam : Adm::F32Sgd;
    if (e.mp && !(admitted(p, base, Adm::Many) && admitted(p, base, Adm::One))) return false;
    if (e.wide || !e.bf16) return admitted(p, e.kind(), Adm::Many) && admitted(p, e.kind(), Adm::One);
    return admitted(p, e.kind(), world == 1 ? Adm::One : Adm::Many);
}

// psgd_aggregate_mixed's ingest fold on `step`: its only gradient pass is the single-pass final
// kernel and that instance is admitted (after eligible())
bool ingest_fold(psgd_plan* p, int64_t step) {
    (void)admitted(p, Adm::Bf16Ingest, Adm::NoComm);
    return p->adm.ok[Adm::Bf16Ingest][Adm::NoComm][step & 1];
}

// A query: admission is a property of this build's kernels on the device, cached in the plan per
// tiling. A plan with no device yet answers for the current device and keeps nothing
template <typename Read>
int query(const psgd_plan* plan, Read read) {
    psgd_plan* p = const_cast<psgd_plan*>(plan);
    DevScope scope(p->device);
    read(p);
    if (!p->bound) p->adm = Adm{};
    return PSGD_OK;
}

// ------------------------------------------------------------------ side state ------
// made once, by the first call on a bound plan: the tables of the plan's tensors and, for the bf16
// sinks, the run-table ADD with its workspace
int ensure(psgd_plan* p, psgd_plan::Side*& slot, bool add) {
    if (slot) return PSGD_OK;
    slot = new psgd_plan::Side();
    const size_t nt = p->shapes.size();
    if (int st = slot->per.room(nt, nullptr)) return st;
    if (!add) return PSGD_OK;
    std::vector<int64_t> zero(nt, 0), numel(nt, 1);
    std::vector<int32_t> idx(nt);
    for (size_t i = 0; i < nt; ++i) {
        idx[i] = int32_t(i);
        for (int64_t x : p->shapes[i]) numel[i] *= x;
    }
    if (int st = psgd_runs_create_mixed(zero.data(), idx.data(), zero.data(), numel.data(), idx.data(), int32_t(nt),
                                        int32_t(nt), int32_t(nt), PSGD_BF16, PSGD_F32, &slot->add))
        return st;
    int64_t rb = 0;
    if (int st = psgd_runs_workspace_bytes(slot->add, &rb)) return st;
    PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&slot->add_ws), size_t(std::max<int64_t>(rb, 1))));
    return psgd_runs_bind(slot->add, p->device, slot->add_ws);
}

void release(psgd_plan::Side*& slot) {
    if (!slot) return;
    if (slot->add) (void)psgd_runs_destroy(slot->add);
    if (slot->add_ws) (void)hipFree(slot->add_ws);
    delete slot;
    slot = nullptr;
}

// ------------------------------------------------------------------ entries ------
// The checks before any device work, in the entry's documented order (include/psgd.h): the exchange
// entries report the argument errors before the plan's state, the others "not bound" before the
// range check; the fp32 tables the plan's shape before the flat plan, the bf16 sinks after it.
// Leaves c.f null where there is no flat tail
int preamble(const Entry& e, Call& c) {
    const psgd_plan* p = c.p;
    const bool args = p && c.state && c.peer && (e.tables || c.out) &&
                      (e.via != Entry::Comm || c.comm || e.upd() || e.wide_dst()) &&
                      (!e.sgd || c.hyper) && (!e.adam || (c.bufs && c.vs && c.adam)) && (!e.mp || (c.grads16 && c.ws));
    if (e.via == Entry::Xchg) {
        if (!args) return fail(PSGD_ERR_VALUE, "null argument");
        if (c.step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
        if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    } else if (int st = check_call(args, p && p->bound, c.step >= 0, "step out of range")) {
        return st;
    }
    if (!e.tables)
        if (int st = check_out(c.out)) return st;
    int code = PSGD_ERR_VALUE;
    const char* why = ineligible(p, e.bf16, e.wide, &code, e.sgd, e.adam, e.wide_dst());
    if (why && !e.bf16) return fail(code, why);
    if (!c.f || c.f->total == 0) c.f = nullptr;
    if (const psgd_flat* f = c.f) {
        const bool type_ok = f->dtype == PSGD_F32 && f->device == p->device;
        std::string msg;  // built for the refusal only: nothing is allocated on a call that passes
        if (!type_ok)
            msg = std::string(e.name) + " takes an fp32 flat plan" + (e.bf16 ? " (the uncompressed tensors' residual)" : "") +
                  " on the codec's device";
        if (int st = check_flat(f, c.unc_state && c.unc_peer && (e.tables || c.flat_out), type_ok, PSGD_ERR_VALUE, msg.c_str()))
            return st;
        if (!e.bf16)
            for (int32_t i = 0; i < f->count; ++i)
                if (!c.unc_state[i] || !c.unc_peer[i]) return fail(PSGD_ERR_VALUE, "null uncompressed tensor pointer");
    }
    if (why) return fail(code, why);
    // every tensor's two pointers: the bf16 side (gradients, or destinations like them) 2-byte
    // aligned and the fp32 residual 4-byte; fp32 destinations 4-byte
    const uintptr_t al = e.bf16 ? 2 : 4;
    const char* al_msg = e.bf16  ? "bf16 gradients must be 2-byte aligned"
                         : e.upd() ? "parameters must be 4-byte aligned"
                                 : "fp32 destinations must be 4-byte aligned";
    for (size_t i = 0; i < p->shapes.size(); ++i) {
        if (!c.state[i] || !c.peer[i]) return fail(PSGD_ERR_VALUE, "null gradient pointer");
        if (reinterpret_cast<uintptr_t>(c.peer[i]) % al) return fail(PSGD_ERR_LAYOUT, al_msg);
        if (e.bf16 && reinterpret_cast<uintptr_t>(c.state[i]) % 4)
            return fail(PSGD_ERR_LAYOUT, "the fp32 residual must be 4-byte aligned");
    }
    if (c.f && !e.bf16)
        for (int32_t i = 0; i < c.f->count; ++i)
            if (reinterpret_cast<uintptr_t>(c.unc_peer[i]) % al) return fail(PSGD_ERR_LAYOUT, al_msg);
    if (e.sgd)
        if (int st = sgd_check(p, c.bufs, c.f, c.unc_bufs, c.hyper)) return st;
    if (e.adam)
        if (int st = adam_check(p, c.bufs, c.vs, c.f, c.unc_bufs, c.unc_vs)) return st;
    if (e.mp)
        if (int st = adam_mp_check(p, c.grads16, c.ws, c.f, c.unc_grads16, c.unc_ws)) return st;
    if (e.via == Entry::Xchg) {
        if (int st = ipc_check(p, c.step)) return st;
        if (c.f && c.f->total > p->ipc_flat_cap)
            return fail(PSGD_ERR_VALUE, "flat tensors exceed the exchange buffer (psgd_ipc_create)");
    }
    return PSGD_OK;
}

// Past the checks. Everything that can refuse comes before the first launch; *refused: the plan has
// no admitted instance (nothing launched, no collective issued: a communicator stays usable)
int body(const Entry& e, const Call& c, bool* refused) {
    psgd_plan* p = c.p;
    psgd_flat* f = c.f;
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    DevScope scope(p->device);
    if (e.upd()) {  // its tables are psgd_plan::Sgd's / Adam's (psgd_sgd.cpp, psgd_adam.cpp), and there is
                    // no transport but the communicator
        if (int st = refresh_pointers(p, c.state, s)) return st;
        if (!eligible(p, e, c.comm ? comm_world(c.comm) : 1)) {  // the narrow entries ask both kinds
            *refused = true;
            return fail(PSGD_ERR_VALUE, std::string(e.name) + ": no admitted update instance of this plan's final pass "
                                                              "(two waves per SIMD, no scratch)");
        }
        OutSink sink;
        if (e.adam) {
            if (int st = adam_select(p, c.peer, c.bufs, c.vs, f, c.unc_peer, c.unc_bufs, c.unc_vs, c.adam, s, &sink))
                return st;
            if (e.mp) {  // the model tensors' tables; then the ADD over every tensor, the first launches
                if (int st = adam_mp_select(p, c.ws, f, c.unc_ws, s, &sink)) return st;
                if (int st = ensure(p, p->mixed, true)) return st;
                if (int st = psgd_runs_add_list(p->mixed->add, c.grads16, c.state, 1, s)) return st;
                if (int st = adam_mp_add(p, f, c.unc_grads16, c.unc_state, s)) return st;
            }
        } else {
            if (int st = sgd_select(p, c.peer, c.bufs, f, c.unc_peer, c.unc_bufs, c.hyper, s, &sink)) return st;
            if (e.mp) {  // as the Adam form above
                if (int st = sgd_mp_select(p, c.ws, f, c.unc_ws, s, &sink)) return st;
                if (int st = ensure(p, p->mixed, true)) return st;
                if (int st = psgd_runs_add_list(p->mixed->add, c.grads16, c.state, 1, s)) return st;
                if (int st = sgd_mp_add(p, f, c.unc_grads16, c.unc_state, s)) return st;
            }
        }
        return aggregate_comm_ctx(p, c.state, c.step, f, c.unc_state, c.comm, s, sink);
    }
    psgd_plan::Side*& slot = e.bf16 ? p->mixed : p->direct;
    if (int st = ensure(p, slot, e.bf16)) return st;
    psgd_plan::Side& m = *slot;
    // the tiling the step will run on: the state's alignment decides the vector layout (a
    // destination's only picks the store form, in the kernel), and admission asks about that tiling.
    // The wide kernels test each tensor's alignment themselves
    if (!e.wide)
        if (int st = refresh_pointers(p, c.state, s)) return st;
    const int world = e.via == Entry::Comm ? (c.comm ? comm_world(c.comm) : 1) : e.via == Entry::Xchg ? p->ipc_world : 1;
    if (!eligible(p, e, world)) {
        *refused = true;
        const char* what = e.wide_dst() ? "k_wide_apply_dst for this plan's rank bucket"
                           : e.wide   ? "k_wide_apply_mix for this plan's rank bucket"
                           : e.tables ? "destination-table instance of this plan's final pass"
                                      : "bf16-output instance of this plan's final pass";
        return fail(PSGD_ERR_VALUE, std::string(e.name) + ": no admitted " + what + " (two waves per SIMD, no scratch)");
    }
    const bool ingest = e.via == Entry::World1 && !e.wide && ingest_fold(p, c.step);
    OutSink sink;
    sink.bf16 = e.bf16;
    sink.tables = e.tables;
    sink.out = c.out;
    sink.flat_out = c.flat_out;
    if (f) {
        if (int st = m.unc.room(size_t(f->count), s)) return st;
        if (e.bf16)
            for (int32_t i = 0; i < f->count; ++i)
                if (!c.unc_peer[i] || !c.unc_state[i]) return fail(PSGD_ERR_VALUE, "null uncompressed tensor pointer");
        // a collective sums fp32: the flat tail is staged, but where it lives in the exchange slot
        // and k_xchg_mix stores its sums as bf16, or rides in the world-size-1 final pass
        if (!e.bf16 || e.via == Entry::Comm || e.wide) {
            if (int st = m.unc.stage_room(size_t(f->total), s)) return st;
            sink.stage = m.unc.stage;
        }
        TableCache& t = e.tables ? m.unc.b : m.unc.a;
        PSGD_HIP(t.select(c.unc_peer, s));
        (e.tables ? sink.unc_dst : sink.unc_src) = t.table();
    }
    if (e.tables) {
        PSGD_HIP(m.per.b.select(c.peer, s));
        sink.dst = m.per.b.table();
    } else if (ingest) {
        PSGD_HIP(m.per.a.select(c.peer, s));
        sink.src = m.per.a.table();
    } else if (int st = psgd_runs_add_list(m.add, c.peer, c.state, 1, s)) {
        return st;
    }
    if (e.via == Entry::Xchg) return aggregate_ipc_ctx(p, c.state, c.step, f, c.unc_state, s, sink);
    if (e.via == Entry::Comm || e.wide) return aggregate_comm_ctx(p, c.state, c.step, f, c.unc_state, c.comm, s, sink);
    FlatArgs fa{};
    StepCtx x = out_ctx(&sink);
    x.mix_in = ingest;
    x.out = c.out;
    if (f) {
        if (int st = flat_args(f, c.unc_state, c.flat_out, 1, s, &fa)) return st;
        x.fl = &fa;
    }
    return aggregate_ctx(p, c.state, c.step, s, x);
}

int run(const Entry& e, Call c) {
    if (int st = preamble(e, c)) return st;
    if (e.via == Entry::Comm && c.comm) return with_comm(c.comm, [&](bool* refused) { return body(e, c, refused); });
    bool refused = false;
    return body(e, c, &refused);
}

// what the queries check of their arguments (`world` 1 where the query takes none)
int query_args(bool ptrs, int64_t step, int32_t world) {
    if (!ptrs) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    if (world < 1) return fail(PSGD_ERR_VALUE, "world size must be >= 1");
    return PSGD_OK;
}

const Entry kMixedFlat{"psgd_aggregate_mixed_flat", Entry::World1, false, false, true};
const Entry kMixedComm{"psgd_aggregate_mixed_comm", Entry::Comm, false, false, true};
const Entry kMixedIpc{"psgd_aggregate_mixed_ipc", Entry::Xchg, false, false, true};
const Entry kMixedWide{"psgd_aggregate_mixed_wide", Entry::World1, true, false, true};
const Entry kMixedWideComm{"psgd_aggregate_mixed_wide_comm", Entry::Comm, true, false, true};
const Entry kMixedCommDst{"psgd_aggregate_mixed_comm_dst", Entry::Comm, false, true, true};
const Entry kMixedIpcDst{"psgd_aggregate_mixed_ipc_dst", Entry::Xchg, false, true, true};
const Entry kCommDst{"psgd_aggregate_comm_dst", Entry::Comm, false, true, false};
const Entry kIpcDst{"psgd_aggregate_ipc_dst", Entry::Xchg, false, true, false};
const Entry kCommSgd{"psgd_aggregate_comm_sgd", Entry::Comm, false, true, false, true};
const Entry kCommAdam{"psgd_aggregate_comm_adam", Entry::Comm, false, true, false, false, true};
const Entry kMixedCommAdam{"psgd_aggregate_mixed_comm_adam", Entry::Comm, false, true, false, false, true, true};
const Entry kCommAdamWide{"psgd_aggregate_comm_adam_wide", Entry::Comm, true, true, false, false, true};
const Entry kMixedCommAdamWide{"psgd_aggregate_mixed_comm_adam_wide", Entry::Comm, true, true, false, false, true, true};
const Entry kCommSgdWide{"psgd_aggregate_comm_sgd_wide", Entry::Comm, true, true, false, true};
const Entry kMixedCommSgd{"psgd_aggregate_mixed_comm_sgd", Entry::Comm, false, true, false, true, false, true};
const Entry kMixedCommSgdWide{"psgd_aggregate_mixed_comm_sgd_wide", Entry::Comm, true, true, false, true, false, true};
const Entry kCommDstWide{"psgd_aggregate_comm_dst_wide", Entry::Comm, true, true, false};
const Entry kMixedCommDstWide{"psgd_aggregate_mixed_comm_dst_wide", Entry::Comm, true, true, true};

}  // namespace

void psgd::side_release(psgd_plan* p) {
    release(p->mixed);
    release(p->direct);
}

bool psgd::direct_shape_ok(const psgd_plan* p) {
    int code = 0;
    return ineligible(p, false, false, &code) == nullptr;
}

int psgd::direct_select(psgd_plan* p, void* const* dst, const psgd_flat* f, void* const* unc_dst, hipStream_t s,
                        DirectDst* t) {
    if (f) {  // checked before the state is made: a refusal leaves nothing behind
        const psgd_plan::Side* m = p->direct;
        if (!m || !m->unc.stage || m->unc.stage_cap < size_t(f->total) || m->unc.cap < size_t(f->count))
            return fail(PSGD_ERR_STATE, "the flat tail is not staged (call after psgd_aggregate_comm_dst / _ipc_dst)");
    }
    if (int st = ensure(p, p->direct, false)) return st;
    psgd_plan::Side& m = *p->direct;
    if (f) {
        if (int st = m.unc.room(size_t(f->count), s)) return st;  // within its capacity: a re-bind at the most
        PSGD_HIP(m.unc.b.select(unc_dst, s));
        t->unc_dst = m.unc.b.table();
        t->stage = m.unc.stage;
    }
    PSGD_HIP(m.per.b.select(dst, s));
    t->dst = m.per.b.table();
    return PSGD_OK;
}

extern "C" {

int psgd_plan_mixed_folds(const psgd_plan* plan, int64_t step, int32_t* fold_in, int32_t* fold_out) {
    if (int st = query_args(plan && fold_in && fold_out, step, 1)) return st;
    *fold_in = *fold_out = 0;
    int code = 0;
    if (ineligible(plan, true, false, &code)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) {
        *fold_out = eligible(p, kMixedFlat, 1) ? 1 : 0;
        *fold_in = *fold_out && ingest_fold(p, step) ? 1 : 0;
    });
}

int psgd_plan_mixed_folds_comm(const psgd_plan* plan, int64_t step, int32_t world, int32_t* fold_in,
                               int32_t* fold_out) {
    if (int st = query_args(plan && fold_in && fold_out, step, world)) return st;
    *fold_in = *fold_out = 0;  // no ingest fold in this form: the ADD is always a launch of its own
    int code = 0;
    if (ineligible(plan, true, false, &code)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *fold_out = eligible(p, kMixedComm, world) ? 1 : 0; });
}

int psgd_plan_mixed_folds_dst(const psgd_plan* plan, int64_t step, int32_t world, int32_t* fold_out) {
    if (int st = query_args(plan && fold_out, step, world)) return st;
    *fold_out = 0;
    int code = 0;
    if (ineligible(plan, true, false, &code)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *fold_out = eligible(p, kMixedCommDst, world) ? 1 : 0; });
}

int psgd_plan_mixed_wide_ok(const psgd_plan* plan, int32_t world, int32_t* ok) {
    if (int st = query_args(plan && ok, 0, world)) return st;
    *ok = 0;
    int code = 0;
    if (ineligible(plan, true, true, &code)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kMixedWideComm, world) ? 1 : 0; });
}

int psgd_plan_dst_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, false, &code)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kCommDst, world) ? 1 : 0; });
}

int psgd_plan_sgd_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t momentum_used, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    if (momentum_used != 0 && momentum_used != 1) return fail(PSGD_ERR_VALUE, "momentum_used is 0 or 1");
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, false, &code, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kCommSgd, world) ? 1 : 0; });
}

int psgd_aggregate_comm_sgd(psgd_plan* p, void* const* grads, void* const* params, void* const* bufs,
                            const psgd_sgd_hyper* hyper, int64_t step, psgd_flat* f, void* const* unc,
                            void* const* unc_params, void* const* unc_bufs, psgd_comm* comm, void* stream) {
    Call c{p, grads, params, nullptr, step, f, unc, unc_params, nullptr, comm, stream};
    c.bufs = bufs;
    c.unc_bufs = unc_bufs;
    c.hyper = hyper;
    return run(kCommSgd, c);
}

int psgd_plan_sgd_wide_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t momentum_used, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    if (momentum_used != 0 && momentum_used != 1) return fail(PSGD_ERR_VALUE, "momentum_used is 0 or 1");
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, true, &code, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kCommSgdWide, world) ? 1 : 0; });
}

int psgd_aggregate_comm_sgd_wide(psgd_plan* p, void* const* grads, void* const* params, void* const* bufs,
                                 const psgd_sgd_hyper* hyper, int64_t step, psgd_flat* f, void* const* unc,
                                 void* const* unc_params, void* const* unc_bufs, psgd_comm* comm, void* stream) {
    Call c{p, grads, params, nullptr, step, f, unc, unc_params, nullptr, comm, stream};
    c.bufs = bufs;
    c.unc_bufs = unc_bufs;
    c.hyper = hyper;
    return run(kCommSgdWide, c);
}

int psgd_plan_mixed_sgd_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t momentum_used, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    if (momentum_used != 0 && momentum_used != 1) return fail(PSGD_ERR_VALUE, "momentum_used is 0 or 1");
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, false, &code, true)) return PSGD_OK;
    // rank bucket 8 with 2 or 3 iterations: its update instances are the ones no fused step admits
    // (the register-cached two-set tile at the scratch edge); answered here without asking the device
    if (plan->rbucket == 8 && (plan->iters == 2 || plan->iters == 3)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kMixedCommSgd, world) ? 1 : 0; });
}

int psgd_plan_mixed_sgd_wide_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t momentum_used, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    if (momentum_used != 0 && momentum_used != 1) return fail(PSGD_ERR_VALUE, "momentum_used is 0 or 1");
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, true, &code, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kMixedCommSgdWide, world) ? 1 : 0; });
}

namespace {

int mixed_comm_sgd(const Entry& e, psgd_plan* p, void* const* grads_bf16, void* const* residual, void* const* params_bf16,
                   void* const* masters, void* const* bufs, const psgd_sgd_hyper* hyper, int64_t step, psgd_flat* f,
                   void* const* unc_bf16, void* const* unc_residual, void* const* unc_params_bf16,
                   void* const* unc_masters, void* const* unc_bufs, psgd_comm* comm, void* stream) {
    Call c{p, residual, masters, nullptr, step, f, unc_residual, unc_masters, nullptr, comm, stream};
    c.bufs = bufs;
    c.unc_bufs = unc_bufs;
    c.hyper = hyper;
    c.grads16 = grads_bf16;
    c.unc_grads16 = unc_bf16;
    c.ws = params_bf16;
    c.unc_ws = unc_params_bf16;
    return run(e, c);
}

}  // namespace

int psgd_aggregate_mixed_comm_sgd(psgd_plan* p, void* const* grads_bf16, void* const* residual,
                                  void* const* params_bf16, void* const* masters, void* const* bufs,
                                  const psgd_sgd_hyper* hyper, int64_t step, psgd_flat* f, void* const* unc_bf16,
                                  void* const* unc_residual, void* const* unc_params_bf16, void* const* unc_masters,
                                  void* const* unc_bufs, psgd_comm* comm, void* stream) {
    return mixed_comm_sgd(kMixedCommSgd, p, grads_bf16, residual, params_bf16, masters, bufs, hyper, step, f, unc_bf16,
                          unc_residual, unc_params_bf16, unc_masters, unc_bufs, comm, stream);
}

int psgd_aggregate_mixed_comm_sgd_wide(psgd_plan* p, void* const* grads_bf16, void* const* residual,
                                       void* const* params_bf16, void* const* masters, void* const* bufs,
                                       const psgd_sgd_hyper* hyper, int64_t step, psgd_flat* f, void* const* unc_bf16,
                                       void* const* unc_residual, void* const* unc_params_bf16,
                                       void* const* unc_masters, void* const* unc_bufs, psgd_comm* comm, void* stream) {
    return mixed_comm_sgd(kMixedCommSgdWide, p, grads_bf16, residual, params_bf16, masters, bufs, hyper, step, f,
                          unc_bf16, unc_residual, unc_params_bf16, unc_masters, unc_bufs, comm, stream);
}

int psgd_plan_adam_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, false, &code, false, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kCommAdam, world) ? 1 : 0; });
}

int psgd_aggregate_comm_adam(psgd_plan* p, void* const* grads, void* const* params, void* const* ms, void* const* vs,
                             const psgd_adam_hyper* hyper, int64_t step, psgd_flat* f, void* const* unc,
                             void* const* unc_params, void* const* unc_ms, void* const* unc_vs, psgd_comm* comm,
                             void* stream) {
    Call c{p, grads, params, nullptr, step, f, unc, unc_params, nullptr, comm, stream};
    c.bufs = ms;
    c.unc_bufs = unc_ms;
    c.vs = vs;
    c.unc_vs = unc_vs;
    c.adam = hyper;
    return run(kCommAdam, c);
}

int psgd_plan_mixed_adam_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, false, &code, false, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kMixedCommAdam, world) ? 1 : 0; });
}

int psgd_aggregate_mixed_comm_adam(psgd_plan* p, void* const* grads_bf16, void* const* residual,
                                   void* const* params_bf16, void* const* masters, void* const* ms, void* const* vs,
                                   const psgd_adam_hyper* hyper, int64_t step, psgd_flat* f, void* const* unc_bf16,
                                   void* const* unc_residual, void* const* unc_params_bf16, void* const* unc_masters,
                                   void* const* unc_ms, void* const* unc_vs, psgd_comm* comm, void* stream) {
    Call c{p, residual, masters, nullptr, step, f, unc_residual, unc_masters, nullptr, comm, stream};
    c.bufs = ms;
    c.unc_bufs = unc_ms;
    c.vs = vs;
    c.unc_vs = unc_vs;
    c.adam = hyper;
    c.grads16 = grads_bf16;
    c.unc_grads16 = unc_bf16;
    c.ws = params_bf16;
    c.unc_ws = unc_params_bf16;
    return run(kMixedCommAdam, c);
}

int psgd_plan_adam_wide_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, true, &code, false, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kCommAdamWide, world) ? 1 : 0; });
}

int psgd_aggregate_comm_adam_wide(psgd_plan* p, void* const* grads, void* const* params, void* const* ms,
                                  void* const* vs, const psgd_adam_hyper* hyper, int64_t step, psgd_flat* f,
                                  void* const* unc, void* const* unc_params, void* const* unc_ms, void* const* unc_vs,
                                  psgd_comm* comm, void* stream) {
    Call c{p, grads, params, nullptr, step, f, unc, unc_params, nullptr, comm, stream};
    c.bufs = ms;
    c.unc_bufs = unc_ms;
    c.vs = vs;
    c.unc_vs = unc_vs;
    c.adam = hyper;
    return run(kCommAdamWide, c);
}

int psgd_plan_mixed_adam_wide_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, true, &code, false, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kMixedCommAdamWide, world) ? 1 : 0; });
}

int psgd_aggregate_mixed_comm_adam_wide(psgd_plan* p, void* const* grads_bf16, void* const* residual,
                                        void* const* params_bf16, void* const* masters, void* const* ms,
                                        void* const* vs, const psgd_adam_hyper* hyper, int64_t step, psgd_flat* f,
                                        void* const* unc_bf16, void* const* unc_residual, void* const* unc_params_bf16,
                                        void* const* unc_masters, void* const* unc_ms, void* const* unc_vs,
                                        psgd_comm* comm, void* stream) {
    Call c{p, residual, masters, nullptr, step, f, unc_residual, unc_masters, nullptr, comm, stream};
    c.bufs = ms;
    c.unc_bufs = unc_ms;
    c.vs = vs;
    c.unc_vs = unc_vs;
    c.adam = hyper;
    c.grads16 = grads_bf16;
    c.unc_grads16 = unc_bf16;
    c.ws = params_bf16;
    c.unc_ws = unc_params_bf16;
    return run(kMixedCommAdamWide, c);
}

int psgd_aggregate_mixed_flat(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16, int64_t step,
                              psgd_flat* f, void* const* unc_bf16, void* const* unc_residual, void* flat_out_bf16,
                              void* stream) {
    return run(kMixedFlat, Call{p, residual, grads_bf16, out_bf16, step, f, unc_residual, unc_bf16, flat_out_bf16,
                                nullptr, stream});
}

int psgd_aggregate_mixed(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16, int64_t step,
                         void* stream) {
    return psgd_aggregate_mixed_flat(p, grads_bf16, residual, out_bf16, step, nullptr, nullptr, nullptr, nullptr,
                                     stream);
}

int psgd_aggregate_mixed_comm(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16,
                              int64_t step, psgd_flat* f, void* const* unc_bf16, void* const* unc_residual,
                              void* flat_out_bf16, psgd_comm* comm, void* stream) {
    return run(kMixedComm, Call{p, residual, grads_bf16, out_bf16, step, f, unc_residual, unc_bf16, flat_out_bf16,
                                comm, stream});
}

int psgd_aggregate_mixed_ipc(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16, int64_t step,
                             psgd_flat* f, void* const* unc_bf16, void* const* unc_residual, void* flat_out_bf16,
                             void* stream) {
    return run(kMixedIpc, Call{p, residual, grads_bf16, out_bf16, step, f, unc_residual, unc_bf16, flat_out_bf16,
                               nullptr, stream});
}

int psgd_aggregate_mixed_wide(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16, int64_t step,
                              psgd_flat* f, void* const* unc_bf16, void* const* unc_residual, void* flat_out_bf16,
                              void* stream) {
    return run(kMixedWide, Call{p, residual, grads_bf16, out_bf16, step, f, unc_residual, unc_bf16, flat_out_bf16,
                                nullptr, stream});
}

int psgd_aggregate_mixed_wide_comm(psgd_plan* p, void* const* grads_bf16, void* const* residual, void* out_bf16,
                                   int64_t step, psgd_flat* f, void* const* unc_bf16, void* const* unc_residual,
                                   void* flat_out_bf16, psgd_comm* comm, void* stream) {
    return run(kMixedWideComm, Call{p, residual, grads_bf16, out_bf16, step, f, unc_residual, unc_bf16,
                                    flat_out_bf16, comm, stream});
}

int psgd_aggregate_mixed_comm_dst(psgd_plan* p, void* const* residual, void* const* dst_bf16, int64_t step,
                                  psgd_flat* f, void* const* unc_residual, void* const* unc_dst_bf16, psgd_comm* comm,
                                  void* stream) {
    return run(kMixedCommDst, Call{p, residual, dst_bf16, nullptr, step, f, unc_residual, unc_dst_bf16, nullptr,
                                   comm, stream});
}

int psgd_aggregate_mixed_ipc_dst(psgd_plan* p, void* const* residual, void* const* dst_bf16, int64_t step, psgd_flat* f,
                                 void* const* unc_residual, void* const* unc_dst_bf16, void* stream) {
    return run(kMixedIpcDst, Call{p, residual, dst_bf16, nullptr, step, f, unc_residual, unc_dst_bf16, nullptr,
                                  nullptr, stream});
}

int psgd_aggregate_comm_dst(psgd_plan* p, void* const* grads, void* const* dst, int64_t step, psgd_flat* f,
                            void* const* unc, void* const* unc_dst, psgd_comm* comm, void* stream) {
    return run(kCommDst, Call{p, grads, dst, nullptr, step, f, unc, unc_dst, nullptr, comm, stream});
}

int psgd_aggregate_ipc_dst(psgd_plan* p, void* const* grads, void* const* dst, int64_t step, psgd_flat* f,
                           void* const* unc, void* const* unc_dst, void* stream) {
    return run(kIpcDst, Call{p, grads, dst, nullptr, step, f, unc, unc_dst, nullptr, nullptr, stream});
}

int psgd_plan_dst_wide_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    *ok = 0;
    int code = 0;
    if (ineligible(plan, false, true, &code, false, false, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kCommDstWide, world) ? 1 : 0; });
}

int psgd_aggregate_comm_dst_wide(psgd_plan* p, void* const* grads, void* const* dst, int64_t step, psgd_flat* f,
                                 void* const* unc, void* const* unc_dst, psgd_comm* comm, void* stream) {
    return run(kCommDstWide, Call{p, grads, dst, nullptr, step, f, unc, unc_dst, nullptr, comm, stream});
}

int psgd_plan_mixed_dst_wide_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok) {
    if (int st = query_args(plan && ok, step, world)) return st;
    *ok = 0;
    int code = 0;
    if (ineligible(plan, true, true, &code, false, false, true)) return PSGD_OK;
    return query(plan, [&](psgd_plan* p) { *ok = eligible(p, kMixedCommDstWide, world) ? 1 : 0; });
}

int psgd_aggregate_mixed_comm_dst_wide(psgd_plan* p, void* const* residual, void* const* dst_bf16, int64_t step,
                                       psgd_flat* f, void* const* unc_residual, void* const* unc_dst_bf16,
                                       psgd_comm* comm, void* stream) {
    return run(kMixedCommDstWide, Call{p, residual, dst_bf16, nullptr, step, f, unc_residual, unc_dst_bf16, nullptr,
                                       comm, stream});
}

}  // extern "C"
