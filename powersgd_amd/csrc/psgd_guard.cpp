// psgd_guard_outputs (include/psgd.h): skip a non-finite step on the device. The driver checks its
// arguments, selects the device table of the gradient pointers (change-detected, TableCache) and
// launches k_guard_check over the plan's bound P / Q state and the dense uncompressed slab, then
// k_guard_apply, which reads the verdict on the device and returns at once on a finite step. No host
// synchronisation: the flag word is never cleared (every call of a plan takes the next epoch, a
// finding workgroup raises the word to it, the consumer tests word == epoch).
#include <cstring>

#include "psgd_guard.h"
#include "psgd_plan.h"

// State of its own like psgd_plan::Norm: one device allocation made by the first call, freed with
// the plan; the caller's workspace carve does not move.
struct psgd_plan::Guard {
    std::vector<GuardItem> items;  // the gradient tensors' bytes in units, tensor order (built once)
    char* dev = nullptr;
    size_t o_flag = 0, o_items = 0, o_tab = 0;
    TableCache tab;                // device tables of the gradient pointers
    unsigned long long epoch = 0;
};

namespace psgd {

void guard_release(psgd_plan* p) {
    if (!p->guard) return;
    p->guard->tab.release();
    if (p->guard->dev) (void)hipFree(p->guard->dev);
    delete p->guard;
    p->guard = nullptr;
}

namespace {

size_t elem_size(int dtype) { return dtype == PSGD_BF16 ? 2 : dtype == PSGD_F64 ? 8 : 4; }

int guard_state(psgd_plan* p) {
    if (p->guard) return PSGD_OK;
    auto* g = new psgd_plan::Guard();
    const size_t esz = elem_size(p->dtype);
    for (size_t i = 0; i < p->shapes.size(); ++i) {
        int64_t bytes = int64_t(esz);
        for (int64_t d : p->shapes[i]) bytes *= d;
        for (int64_t o = 0; o < bytes; o += kGuardUnit)
            g->items.push_back(GuardItem{o, int32_t(i), int32_t(std::min<int64_t>(kGuardUnit, bytes - o))});
    }
    size_t off = 0;
    auto carve = [&off](size_t bytes) {
        const size_t o = off;
        off = align256(off + std::max<size_t>(bytes, 8));
        return o;
    };
    g->o_flag = carve(sizeof(unsigned long long));
    g->o_items = carve(g->items.size() * sizeof(GuardItem));
    g->o_tab = carve(TableCache::bytes(p->shapes.size()));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&g->dev), off);
    if (e != hipSuccess) {
        delete g;
        return fail(PSGD_ERR_DEVICE, std::string("hipMalloc (guard state): ") + hipGetErrorString(e));
    }
    g->tab.bind(g->dev + g->o_tab, p->shapes.size());
    p->guard = g;
    const unsigned long long zero = 0;
    if (int st = upload(g->dev + g->o_flag, &zero, sizeof(zero))) return st;
    return upload(g->dev + g->o_items, g->items.data(), g->items.size() * sizeof(GuardItem));
}

int check_wg(int64_t numel, size_t esz) {  // workgroups of k_guard_check for a range: one batch of loads each at least
    if (numel <= 0) return 0;
    const int64_t per = int64_t(4) * kBlock * (16 / int64_t(esz));
    return int(std::min<int64_t>(kGuardCheckWg, (numel + per - 1) / per));
}

}  // namespace
}  // namespace psgd

extern "C" {

int psgd_guard_outputs(psgd_plan* p, void* const* grads, void* out, void* flat_out, int64_t flat_numel,
                       const void* p_init, const void* q_init, int64_t* result, void* stream) {
    if (!p || !result) return fail(PSGD_ERR_VALUE, "null argument");
    if (out && (!grads || !p_init || !q_init))
        return fail(PSGD_ERR_VALUE, "a compressing step needs grads, p_init and q_init");
    if (flat_numel < 0 || (flat_numel > 0 && !flat_out)) return fail(PSGD_ERR_VALUE, "flat_out / flat_numel mismatch");
    if (!flat_out) flat_numel = 0;
    if (out)
        for (size_t i = 0; i < p->shapes.size(); ++i)
            if (!grads[i]) return fail(PSGD_ERR_VALUE, "null gradient pointer");
    const size_t esz = elem_size(p->dtype), fesz = p->f64() ? 8 : 4;
    auto mis = [](const void* q, size_t a) { return reinterpret_cast<uintptr_t>(q) % a != 0; };
    if (mis(out, esz) || mis(flat_out, esz) || (out && (mis(p_init, fesz) || mis(q_init, fesz))))
        return fail(PSGD_ERR_LAYOUT, "buffers must be aligned to their element size");
    if (mis(result, sizeof(int64_t))) return fail(PSGD_ERR_LAYOUT, "result must be 8-byte aligned");
    if (out)
        for (size_t i = 0; i < p->shapes.size(); ++i)
            if (mis(grads[i], esz)) return fail(PSGD_ERR_LAYOUT, "gradients must be aligned to their element size");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int st = guard_state(p)) return st;
    psgd_plan::Guard* g = p->guard;
    if (out) PSGD_HIP(g->tab.select(grads, s));
    ++g->epoch;
    unsigned long long* flag = reinterpret_cast<unsigned long long*>(g->dev + g->o_flag);

    GuardCheckArgs ca{};
    if (out) {  // a warm-up step has run no codec: P and Q are neither read nor reset
        ca.base[0] = p->P;
        ca.numel[0] = p->ptot;
        ca.base[1] = p->Q;
        ca.numel[1] = p->qtot;
    }
    ca.dtype[0] = ca.dtype[1] = p->f64() ? PSGD_F64 : PSGD_F32;
    ca.base[2] = flat_out;
    ca.numel[2] = flat_numel;
    ca.dtype[2] = p->dtype;
    ca.nwg[0] = check_wg(ca.numel[0], fesz);
    ca.nwg[1] = check_wg(ca.numel[1], fesz);
    ca.nwg[2] = check_wg(ca.numel[2], esz);
    ca.flag = flag;
    ca.epoch = g->epoch;
    PSGD_HIP(launch_guard_check(ca, s));

    GuardApplyArgs aa{};
    if (out) {
        aa.items = reinterpret_cast<const GuardItem*>(g->dev + g->o_items);
        aa.grads = g->tab.table();
        aa.nitems = int64_t(g->items.size());
        aa.zero[0] = out;
        aa.zbytes[0] = p->out_total * int64_t(esz);
        aa.cdst[0] = p->P;
        aa.csrc[0] = p_init;
        aa.cbytes[0] = p->ptot * int64_t(fesz);
        aa.cdst[1] = p->Q;
        aa.csrc[1] = q_init;
        aa.cbytes[1] = p->qtot * int64_t(fesz);
    }
    aa.zero[1] = flat_out;
    aa.zbytes[1] = flat_numel * int64_t(esz);
    aa.esz = int32_t(esz);
    aa.fesz = int32_t(fesz);
    aa.flag = flag;
    aa.epoch = g->epoch;
    aa.result = reinterpret_cast<long long*>(result);
    PSGD_HIP(launch_guard_apply(aa, s));
    return PSGD_OK;
}

}  // extern "C"
