// psgd_clip_outputs / psgd_plan_norm_form (include/psgd.h): global-norm clipping of a step's
// averages. The driver picks the form (factors: two small Gram matrices per compressed matrix from
// the term set the step's output pass recorded in the plan, psgd_plan::norm_rec; stream: a sum of
// squares over the dense outputs), launches the finishing step and, unless max_norm is +inf, the
// scale pass, which reads the coefficient on the device and returns at once when nothing is
// clipped. No host synchronisation.
// psgd_clip_dst / psgd_plan_clip_dst_ok: the same after a direct-store completion
// (psgd_direct.cpp): the factor form and the stream sum over the plan's staged flat tail, then the
// scale pass through the destination tables (k_norm_scale_dst).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "psgd_norm.h"
#include "psgd_plan.h"

// State of its own like psgd_plan::Mixed / Direct: one device allocation made by the first call,
// freed with the plan; the caller's workspace carve does not move.
struct psgd_plan::Norm {
    std::vector<NormItem> items;
    std::vector<NormMat> nmats;
    int ept = 1;
    int64_t part_doubles = 0;
    char* dev = nullptr;
    size_t o_items = 0, o_nmats = 0, o_part = 0, o_sq = 0, o_spart = 0, o_ditems = 0;
    int admitted = -1;  // every instance: at least two waves per SIMD, no scratch (asked once)
    // psgd_clip_dst: the scale items of the plan's tensors (made with the state, from the numels),
    // and those of the flat plan last seen (`fkey`: its entries' tensor and numel), in a second
    // allocation that only another flat plan rebuilds (grown when that one has more items)
    std::vector<NormDstItem> ditems, fitems;
    std::vector<int64_t> fkey;
    bool fhave = false;
    size_t fcap = 0;  // items
    char* fdev = nullptr;
};

namespace psgd {

void norm_release(psgd_plan* p) {
    if (!p->norm) return;
    if (p->norm->dev) (void)hipFree(p->norm->dev);
    if (p->norm->fdev) (void)hipFree(p->norm->fdev);
    delete p->norm;
    p->norm = nullptr;
}

namespace {

enum { kFormAuto = 0, kFormFactors = 1, kFormStream = 2 };

// the factor form serves the plan at all: fp32 factors, ranks up to 32, a stacked width within
// the Gram kernel's
bool factors_static(const psgd_plan* p) {
    return !p->f64() && !p->wide() && p->iters * p->rbucket <= kNormMaxK;
}
bool record_ok(const psgd_plan* p, int64_t step, int32_t world) {
    const psgd_plan::NormRec& r = p->norm_rec;
    return r.have && r.step == step && r.world == world && r.nterms == p->iters;
}

// what auto takes: the stream form wherever the factor form does not apply or PSGD_NORM_FORM
// forces it. An unbound plan has run no step: its answer is the plan's own (static) one.
int auto_form(const psgd_plan* p, int64_t step, int32_t world) {
    if (!factors_static(p) || p->norm_env == kFormStream) return kFormStream;
    if (p->bound && !record_ok(p, step, world)) return kFormStream;
    return kFormFactors;
}

int ept_for(int K) {
    const int ne = K * (K + 1) / 2;
    return ne <= kBlock ? 1 : ne <= 2 * kBlock ? 2 : ne <= 4 * kBlock ? 4 : 9;
}

// the scale items of one destination: [0, numel) in pieces of kNormDstItem elements (none when empty)
void dst_items(std::vector<NormDstItem>& v, int32_t tensor, int64_t numel) {
    for (int64_t o = 0; o < numel; o += kNormDstItem)
        v.push_back(NormDstItem{o, tensor, int32_t(std::min<int64_t>(kNormDstItem, numel - o))});
}

int norm_state(psgd_plan* p) {
    if (p->norm) return PSGD_OK;
    auto* n = new psgd_plan::Norm();
    if (factors_static(p)) {
        int kmax = 1;
        for (const MatDesc& d : p->mats) kmax = std::max(kmax, p->iters * d.r);
        n->ept = ept_for(kmax);
        for (size_t i = 0; i < p->mats.size(); ++i) {
            const MatDesc& d = p->mats[i];
            const int K = p->iters * d.r, ne = K * (K + 1) / 2;
            const int64_t rows_per = ne > 2 * kBlock ? 512 : 256;
            NormMat nm{};
            for (int side = 0; side < 2; ++side) {
                const int64_t rows = side ? d.m : d.n;
                nm.item0[side] = int32_t(n->items.size());
                for (int64_t r0 = 0; r0 < rows; r0 += rows_per) {
                    n->items.push_back(NormItem{int32_t(i), side, int32_t(r0), int32_t(std::min(rows_per, rows - r0)),
                                                n->part_doubles});
                    n->part_doubles += ne;
                }
                nm.nitems[side] = int32_t(n->items.size()) - nm.item0[side];
            }
            n->nmats.push_back(nm);
        }
    }
    if (direct_shape_ok(p))  // psgd_clip_dst's scale items: tensor i of the plan's order, its numel cut in order
        for (size_t i = 0; i < p->shapes.size(); ++i) {
            int64_t numel = 1;
            for (int64_t d : p->shapes[i]) numel *= d;
            dst_items(n->ditems, int32_t(i), numel);
        }
    size_t off = 0;
    auto carve = [&off](size_t bytes) {
        const size_t o = off;
        off = align256(off + std::max<size_t>(bytes, 8));
        return o;
    };
    n->o_items = carve(n->items.size() * sizeof(NormItem));
    n->o_nmats = carve(n->nmats.size() * sizeof(NormMat));
    n->o_part = carve(size_t(n->part_doubles) * sizeof(double));
    n->o_sq = carve(p->shapes.size() * sizeof(double));
    n->o_spart = carve(size_t(2) * kNormStreamWg * sizeof(double));
    n->o_ditems = carve(n->ditems.size() * sizeof(NormDstItem));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&n->dev), off);
    if (e != hipSuccess) {
        delete n;
        return fail(PSGD_ERR_DEVICE, std::string("hipMalloc (norm state): ") + hipGetErrorString(e));
    }
    p->norm = n;
    if (int st = upload(n->dev + n->o_items, n->items.data(), n->items.size() * sizeof(NormItem))) return st;
    if (int st = upload(n->dev + n->o_ditems, n->ditems.data(), n->ditems.size() * sizeof(NormDstItem))) return st;
    return upload(n->dev + n->o_nmats, n->nmats.data(), n->nmats.size() * sizeof(NormMat));
}

int stream_wg(int64_t numel, int64_t per_elems) {  // workgroups of k_norm_stream for a range
    if (numel <= 0) return 0;
    return int(std::min<int64_t>(kNormStreamWg, (numel + per_elems - 1) / per_elems));
}


// The norm of a step's averages and the coefficient into `result` (k_norm_gram + k_norm_mat, or
// k_norm_stream; k_norm_finish): the compressed tensors from the recorded term set (`factors`) or
// from range 0 of `rg`, the dense uncompressed averages from range 1. Shared by psgd_clip_outputs
// and psgd_clip_dst: the same launches on the same arguments give the same bits.
int launch_norm(psgd_plan* p, bool factors, NormRangeArgs rg, size_t esz, double max_norm, double* result,
                hipStream_t s) {
    psgd_plan::Norm* n = p->norm;
    const int64_t per = int64_t(4) * kBlock * (16 / int64_t(esz)) * 4;  // elements per workgroup at least
    rg.nwg[0] = stream_wg(rg.numel[0], per);
    rg.nwg[1] = stream_wg(rg.numel[1], per);
    double* spart = reinterpret_cast<double*>(n->dev + n->o_spart);
    double* sq = reinterpret_cast<double*>(n->dev + n->o_sq);
    if (factors) {
        const psgd_plan::NormRec& rec = p->norm_rec;
        NormGramArgs ga{};
        ga.mats = p->dev(p->mats);
        ga.items = reinterpret_cast<const NormItem*>(n->dev + n->o_items);
        ga.apx = rec.apx;
        ga.nterms = rec.nterms;
        ga.part = reinterpret_cast<double*>(n->dev + n->o_part);
        // (the uncompressed slab's stream-form workgroups ride in this launch)
        PSGD_HIP(launch_norm_gram(n->ept, ga, int(n->items.size()), p->dtype, rg, spart, s));
        NormMatArgs ma{};
        ma.mats = ga.mats;
        ma.items = ga.items;
        ma.nmats = reinterpret_cast<const NormMat*>(n->dev + n->o_nmats);
        ma.part = ga.part;
        ma.nterms = rec.nterms;
        ma.alpha = double(rec.alpha);
        ma.sq = sq;
        PSGD_HIP(launch_norm_mat(ma, int(n->nmats.size()), s));
    }
    if (!factors) PSGD_HIP(launch_norm_stream(p->dtype, rg, spart, s));
    NormFinishArgs fa{};
    fa.sq = factors ? sq : nullptr;
    fa.nsq = factors ? int32_t(p->shapes.size()) : 0;
    fa.part = spart;
    fa.npart[0] = rg.nwg[0];
    fa.npart[1] = rg.nwg[1];
    fa.max_norm = max_norm;
    fa.result = result;
    PSGD_HIP(launch_norm_finish(fa, s));
    return PSGD_OK;
}

// psgd_clip_dst serves the plan: one the direct-store calls serve by shape, the factor form
// applies statically and PSGD_NORM_FORM does not force the stream form. No device is asked.
bool clip_dst_static(const psgd_plan* p) {
    return direct_shape_ok(p) && factors_static(p) && p->norm_env != kFormStream;
}

// the scale items of the flat plan's destinations (table order: FlatEntry::tensor), on the device;
// kept until a flat plan with other tensors comes
int flat_dst_items(psgd_plan::Norm* n, const psgd_flat* f, hipStream_t s) {
    std::vector<int64_t> key;
    key.reserve(2 * f->entries.size());
    for (const FlatEntry& en : f->entries) {
        key.push_back(en.tensor);
        key.push_back(en.numel);
    }
    if (n->fhave && key == n->fkey) return PSGD_OK;
    n->fhave = false;
    n->fitems.clear();
    for (const FlatEntry& en : f->entries) dst_items(n->fitems, int32_t(en.tensor), en.numel);
    PSGD_HIP(hipStreamSynchronize(s));  // an earlier scale launch may still read the old items
    if (n->fitems.size() > n->fcap) {
        if (n->fdev) PSGD_HIP(hipFree(n->fdev));
        n->fdev = nullptr;
        n->fcap = 0;
        PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&n->fdev), n->fitems.size() * sizeof(NormDstItem)));
        n->fcap = n->fitems.size();
    }
    if (int st = upload(n->fdev, n->fitems.data(), n->fitems.size() * sizeof(NormDstItem))) return st;
    n->fkey.swap(key);
    n->fhave = true;
    return PSGD_OK;
}

}  // namespace
}  // namespace psgd

extern "C" {

int psgd_plan_norm_form(const psgd_plan* p, int64_t step, int32_t world, int32_t* form) {
    if (!p || !form) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0 || world < 1) return fail(PSGD_ERR_VALUE, "step/world size out of range");
    *form = auto_form(p, step, world);
    return PSGD_OK;
}

int psgd_clip_outputs(psgd_plan* p, int64_t step, int32_t world, void* out, void* flat_out, int64_t flat_numel,
                      double max_norm, int32_t form, double* result, void* stream) {
    if (int st = check_call(p && result, p && p->bound, step >= 0 && world >= 1, "step/world size out of range"))
        return st;
    if (!(max_norm > 0.0)) return fail(PSGD_ERR_VALUE, "max_norm must be positive");
    if (form < kFormAuto || form > kFormStream) return fail(PSGD_ERR_VALUE, "form must be 0 (auto), 1 (factors) or 2 (stream)");
    if (flat_numel < 0 || (flat_numel > 0 && !flat_out)) return fail(PSGD_ERR_VALUE, "flat_out / flat_numel mismatch");
    if (!flat_out) flat_numel = 0;
    const size_t esz = p->dtype == PSGD_BF16 ? 2 : p->dtype == PSGD_F64 ? 8 : 4;
    if (reinterpret_cast<uintptr_t>(out) % esz || reinterpret_cast<uintptr_t>(flat_out) % esz ||
        reinterpret_cast<uintptr_t>(result) % sizeof(double))
        return fail(PSGD_ERR_LAYOUT, "buffers must be aligned to their element size");
    if (form == kFormFactors) {  // refused before any launch where the factor form does not apply
        if (!factors_static(p))
            return fail(PSGD_ERR_VALUE, "the factor form serves fp32/bf16 plans up to rank 32 with iterations x rank bucket <= 64");
        if (!out) return fail(PSGD_ERR_VALUE, "the factor form needs the step's compressed outputs");
        if (!record_ok(p, step, world))
            return fail(PSGD_ERR_STATE, "no record of this step's output terms (call after its aggregate / decompress)");
    }
    const bool factors = out && (form == kFormFactors || (form == kFormAuto && auto_form(p, step, world) == kFormFactors));
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int st = norm_state(p)) return st;
    psgd_plan::Norm* n = p->norm;
    if (n->admitted < 0) n->admitted = norm_min_waves() >= 2 ? 1 : 0;
    if (!n->admitted) return fail(PSGD_ERR_DEVICE, "a norm kernel instance is not admitted (two waves per SIMD, no scratch)");

    NormRangeArgs rg{};
    rg.base[0] = factors ? nullptr : out;
    rg.numel[0] = factors || !out ? 0 : p->out_total;
    rg.base[1] = flat_out;
    rg.numel[1] = flat_numel;
    if (int st = launch_norm(p, factors, rg, esz, max_norm, result, s)) return st;
    if (std::isinf(max_norm)) return PSGD_OK;  // norm only
    NormRangeArgs sc{};
    sc.base[0] = out;
    sc.numel[0] = out ? p->out_total : 0;
    sc.base[1] = flat_out;
    sc.numel[1] = flat_numel;
    const int64_t ev = int64_t(kNormVecs) * (16 / int64_t(esz));
    for (int k = 0; k < 2; ++k) {
        // one workgroup more than the vectors need when the range is misaligned (head + tail live
        // in workgroup 0 whatever the count); at least one workgroup for a non-empty range
        const int64_t wg = sc.numel[k] > 0 ? (sc.numel[k] + ev - 1) / ev : 0;
        if (wg > (int64_t(1) << 30)) return fail(PSGD_ERR_VALUE, "range too large for the scale pass");
        sc.nwg[k] = int32_t(wg);
    }
    PSGD_HIP(launch_norm_scale(p->dtype, sc, result, s));
    return PSGD_OK;
}

int psgd_plan_clip_dst_ok(const psgd_plan* p, int32_t* ok) {
    if (!p || !ok) return fail(PSGD_ERR_VALUE, "null argument");
    *ok = clip_dst_static(p) ? 1 : 0;
    return PSGD_OK;
}

int psgd_clip_dst(psgd_plan* p, int64_t step, int32_t world, void* const* dst, psgd_flat* f, void* const* unc_dst,
                  double max_norm, double* result, void* stream) {
    if (!p || !dst || !result) return fail(PSGD_ERR_VALUE, "null argument");
    const bool has_flat = f && f->total > 0;
    if (has_flat && !unc_dst) return fail(PSGD_ERR_VALUE, "null argument");
    if (!(max_norm > 0.0)) return fail(PSGD_ERR_VALUE, "max_norm must be positive");
    if (step < 0 || world < 1) return fail(PSGD_ERR_VALUE, "step/world size out of range");
    if (!clip_dst_static(p))
        return fail(PSGD_ERR_VALUE, "psgd_clip_dst serves fp32 plans of one bucket up to rank 32 with iterations x rank "
                                    "bucket <= 64 (psgd_plan_clip_dst_ok)");
    if (has_flat && f->dtype != PSGD_F32) return fail(PSGD_ERR_VALUE, "psgd_clip_dst takes an fp32 flat plan");
    for (size_t i = 0; i < p->shapes.size(); ++i)
        if (!dst[i]) return fail(PSGD_ERR_VALUE, "null destination pointer");
    if (has_flat)
        for (int32_t i = 0; i < f->count; ++i)
            if (!unc_dst[i]) return fail(PSGD_ERR_VALUE, "null uncompressed destination pointer");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    for (size_t i = 0; i < p->shapes.size(); ++i)
        if (reinterpret_cast<uintptr_t>(dst[i]) % 4) return fail(PSGD_ERR_LAYOUT, "fp32 destinations must be 4-byte aligned");
    if (has_flat)
        for (int32_t i = 0; i < f->count; ++i)
            if (reinterpret_cast<uintptr_t>(unc_dst[i]) % 4)
                return fail(PSGD_ERR_LAYOUT, "fp32 destinations must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(result) % sizeof(double)) return fail(PSGD_ERR_LAYOUT, "result must be 8-byte aligned");
    if (!record_ok(p, step, world))
        return fail(PSGD_ERR_STATE, "no record of this step's output terms (call after its psgd_aggregate_comm_dst / _ipc_dst)");
    DevScope scope(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int st = norm_state(p)) return st;
    psgd_plan::Norm* n = p->norm;
    if (n->admitted < 0) n->admitted = norm_min_waves() >= 2 ? 1 : 0;
    if (!n->admitted) return fail(PSGD_ERR_DEVICE, "a norm kernel instance is not admitted (two waves per SIMD, no scratch)");
    // the device tables the direct-store call selected, and the staging its collective summed the
    // flat tail into (refused when it has none for this flat plan)
    DirectDst t{};
    if (int st = direct_select(p, dst, has_flat ? f : nullptr, unc_dst, s, &t)) return st;
    if (has_flat)
        if (int st = flat_dst_items(n, f, s)) return st;

    // The uncompressed averages are read where the copy items read them: the plan's staging buffer,
    // an allocation base holding flat->total floats in the flat plan's layout, exactly what the
    // defining sequence's dense flat slab holds. NormSplit cuts a 16-byte-aligned base of the same
    // length into the same (empty) head, vectors and tail, and the workgroup count depends on the
    // length alone: the partial sums, and so the bits of the norm, are the slab's.
    NormRangeArgs rg{};
    rg.base[1] = has_flat ? t.stage : nullptr;
    rg.numel[1] = has_flat ? f->total : 0;
    if (int st = launch_norm(p, true, rg, sizeof(float), max_norm, result, s)) return st;
    if (std::isinf(max_norm)) return PSGD_OK;  // norm only
    NormDstArgs da{};
    da.items[0] = reinterpret_cast<const NormDstItem*>(n->dev + n->o_ditems);
    da.table[0] = t.dst;
    da.nitems[0] = int32_t(n->ditems.size());
    if (has_flat) {
        da.items[1] = reinterpret_cast<const NormDstItem*>(n->fdev);
        da.table[1] = t.unc_dst;
        da.nitems[1] = int32_t(n->fitems.size());
    }
    PSGD_HIP(launch_norm_scale_dst(da, result, s));
    return PSGD_OK;
}

}  // extern "C"
