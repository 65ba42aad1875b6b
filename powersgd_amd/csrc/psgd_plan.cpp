// Plan lifecycle behind the C ABI of include/psgd.h: create (groups, factor layout, knobs),
// the layout queries, bind, buckets and benchmark timing.
//
// Layout mirrors the reference exactly where it is observable:
//   - matrices = tensor.view(shape[0], -1), grouped by matrix shape in first-appearance order
//     (reference powersgd/powersgd.py:253-263, :283-289);
//   - P state = concat over groups of [count, n, r], Q state = concat of [count, m, r],
//     r = min(rank, n, m) (:130-144, :237-251);
//   - iteration parity = (step * num_iters_per_step + it) % 2 (:174).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>

#include "psgd_plan.h"

namespace {
thread_local std::string g_err;
}

namespace psgd {

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int comm_fail(int code, const char* msg) { return fail(code, msg); }

int64_t env_int(const char* name, int64_t dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return std::atoll(v);
}

int upload(void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return PSGD_OK;
    PSGD_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return PSGD_OK;
}

}  // namespace psgd

psgd_plan::~psgd_plan() {
    for (auto& e : ev_pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    ipc_release(this);
    mixed_release(this);
    direct_release(this);
    norm_release(this);
    guard_release(this);
    if (xerr_host) (void)hipHostFree(xerr_host);
    if (stamp_buf) (void)hipFree(stamp_buf);
}

extern "C" {

int psgd_version(void) { return 102; }

const char* psgd_last_error(void) { return g_err.c_str(); }

int psgd_should_compress(const int64_t* shape, int32_t ndim, int32_t rank, int32_t iters,
                         double min_rate, int32_t* out) {
    if (!shape || !out || ndim < 1) return fail(PSGD_ERR_VALUE, "shape must have at least one dim");
    int64_t numel = 1, sum = 0, mn = shape[0];
    for (int i = 0; i < ndim; ++i) {
        numel *= shape[i];
        sum += shape[i];
        mn = std::min(mn, shape[i]);
    }
    const double r = double(std::min<int64_t>(rank, mn));
    const double avg = 0.5 * double(iters) * r * double(sum);  // reference :292-294
    if (avg == 0.0) return fail(PSGD_ERR_VALUE, "zero average compressed size (division by zero)");
    *out = (double(numel) / avg > min_rate) ? 1 : 0;  // reference :101-105
    return PSGD_OK;
}

int psgd_plan_create(const int64_t* dims, const int32_t* ndims, int32_t num_tensors, int32_t rank,
                     int32_t iters, int32_t dtype, psgd_plan** out_plan) {
    if (!out_plan) return fail(PSGD_ERR_VALUE, "out_plan is null");
    *out_plan = nullptr;
    if (num_tensors < 1 || !dims || !ndims) return fail(PSGD_ERR_INDEX, "list index out of range (no tensors)");
    if (rank < 1) return fail(PSGD_ERR_VALUE, "rank must be >= 1");
    if (iters < 1 || iters > PSGD_MAX_ITERS) return fail(PSGD_ERR_VALUE, "num_iters_per_step must be in [1, 16]");
    if (dtype != PSGD_F32 && dtype != PSGD_BF16 && dtype != PSGD_F64)
        return fail(PSGD_ERR_DTYPE, "dtype must be fp32, bf16 or fp64");

    std::unique_ptr<psgd_plan> p(new psgd_plan());  // freed on every error return
    p->rank = rank;
    p->iters = iters;
    p->dtype = dtype;
    std::map<std::pair<int64_t, int64_t>, int> gid;
    const int64_t* d = dims;
    for (int t = 0; t < num_tensors; ++t) {
        const int nd = ndims[t];
        if (nd < 1) return fail(PSGD_ERR_INDEX, "tuple index out of range (0-dim tensor)");
        std::vector<int64_t> s(d, d + nd);
        d += nd;
        int64_t numel = 1;
        for (int64_t x : s) numel *= x;
        if (numel <= 0) return fail(PSGD_ERR_LAYOUT, "cannot view an empty tensor as a matrix");
        const int64_t n = s[0], m = numel / n;
        auto key = std::make_pair(n, m);
        auto it = gid.find(key);
        if (it == gid.end()) {
            it = gid.emplace(key, int(p->groups.size())).first;
            psgd_plan::Group g;
            g.n = n;
            g.m = m;
            g.r = int(std::min<int64_t>(rank, std::min(n, m)));
            g.poff = g.qoff = 0;
            p->groups.push_back(g);
        }
        p->groups[it->second].tensors.push_back(t);
        p->shapes.push_back(std::move(s));
        // compression_rate bookkeeping (reference :265-275, on the ORIGINAL shape)
        int64_t sum = 0, mn = p->shapes.back()[0];
        for (int64_t x : p->shapes.back()) {
            sum += x;
            mn = std::min(mn, x);
        }
        p->unc_floats += double(numel);
        p->comp_floats += 0.5 * iters * double(std::min<int64_t>(rank, mn)) * double(sum);
    }
    int maxr = 1;
    for (auto& g : p->groups) maxr = std::max(maxr, g.r);
    if (maxr > 32 && dtype == PSGD_F64)
        return fail(PSGD_ERR_VALUE, "effective rank above 32 is not supported for fp64 plans");
    if (maxr > 128) return fail(PSGD_ERR_VALUE, "effective rank above 128 is not supported by this build");
    p->rbucket = int(pow2ceil(maxr));
    {
        int64_t total = 0;
        for (auto& g : p->groups) total += int64_t(g.tensors.size()) * g.n * g.m;
        // about 3k tiles (12 per CU) on large problems, never below 4k elements per tile: the
        // cold even product on ResNet-50 is fastest at 8k-element tiles (profiles/r02/tile_sweep.txt)
        // small plans (<= 4M elements): about one tile per CU (cfg5 4096 x 512: 8192-element
        // tiles 0.038 -> 0.033 ms/step with the final blocks below; profiles/r02b/small)
        const int64_t small = std::min<int64_t>(16384, std::max<int64_t>(4096, total / 256));
        p->tile_elems = total <= (int64_t(1) << 22) ? small : std::min<int64_t>(16384, std::max<int64_t>(4096, total / 3072));
        // Fused final pass: ~1500 row blocks on ResNet-50 (about three rounds of the
        // resident workgroups); the sweeps in profiles/r01 put the optimum at 16-24k
        // elements per block.
        // Rank 1 (256-thread row groups): twice as many, smaller blocks (ResNet-50: ~8k elements,
        // ~3000 blocks): cfg2 0.0818 -> 0.0771 ms, final pass 55.7 -> 51.4 us; rank 4 (512-thread
        // groups) slower there, 0.097 -> 0.103 ms (profiles/r04/g)
        const int64_t per = maxr <= 1 ? 3072 : 1536;
        const int64_t gbytes = total * (p->dtype == PSGD_BF16 ? 2 : p->dtype == PSGD_F64 ? 8 : 4);
        p->out_nt = gbytes > (int64_t(32) << 20) ? 1 : 0;
        p->fin_elems = total <= (int64_t(1) << 22) ? small : std::min<int64_t>(65536, std::max<int64_t>(4096, total / per));
        // the K-term form (world size > 1, and world size 1 beyond two iterations) keeps ~16k at
        // every rank: cfg2 over the multi-GPU code path 0.0932-0.0959 -> 0.0916-0.0918 ms
        // (profiles/r04/o)
        const int64_t dflt_kt = total <= (int64_t(1) << 22) ? small
                                                            : std::min<int64_t>(65536, std::max<int64_t>(4096, total / 1536));
        p->fin_elems_kt = std::max<int64_t>(1024, env_int("PSGD_FIN_ELEMS_KT", dflt_kt));
        // persistent even product: workgroups per CU, minimum gradient elements per workgroup
        // default: the first-iteration instance's resident workgroups per CU (capped at 4), so the
        // grid is one wave of resident workgroups (rank 4: 3 since the narrow-strip path fits 6
        // waves per SIMD; bf16 ranks 2 / 4: 2)
        int resident = p->dtype == PSGD_F32 ? even_resident_f32(p->rbucket) : even_resident_bf16(p->rbucket);
        resident = resident > 0 ? std::min(resident, 4) : 4;
        p->even_wpc = int(std::min<int64_t>(kEvenWpcMax, std::max<int64_t>(1, env_int("PSGD_EVEN_WPC", resident))));
        p->even_min = std::max<int64_t>(1024, env_int("PSGD_EVEN_MIN", 16384));
        // segment cost: rank 4 writes 4 floats per column per segment, so fewer, longer
        // segments pay there (cfg3 k_even 23.3-23.8 -> 22.7 us at 8192); neutral at rank 1
        // (profiles/r04/j)
        p->even_segc = maxr >= 4 ? 8192 : 4096;
    }
    // PSGD_FUSE_FINAL: 0 off; 1 (default) the fused forms of the final pass
    const int64_t fuse_mode = env_int("PSGD_FUSE_FINAL", 1);
    if (fuse_mode != 0 && fuse_mode != 1) {  // 2 was the removed rank-4 K-term form
        static bool warned = false;
        if (!warned)
            std::fprintf(stderr, "psgd: PSGD_FUSE_FINAL=%lld is not a mode (0 or 1); using 1\n",
                         static_cast<long long>(fuse_mode));
        warned = true;
    }
    p->fuse_final_on = fuse_mode != 0;
    p->fin_proj_on = env_int("PSGD_FIN_PROJ", 1) != 0;
    p->oe_on = env_int("PSGD_OE", 1) != 0;
    p->orth_chol = env_int("PSGD_ORTH_CHOL", 1) != 0;
    p->mix_ingest_on = env_int("PSGD_MIXED_INGEST", 1) != 0;
    // PSGD_NORM_FORM=auto|factors|stream: the form psgd_clip_outputs' auto takes (A/B runs); the
    // factor form still runs only where it applies
    if (const char* nf = std::getenv("PSGD_NORM_FORM")) {
        const std::string v(nf);
        if (v == "factors") p->norm_env = 1;
        else if (v == "stream") p->norm_env = 2;
        else if (!v.empty() && v != "auto") return fail(PSGD_ERR_VALUE, "PSGD_NORM_FORM must be auto, factors or stream");
    }

    // output layout: dense, tensor order (what torch.cat / unflatten produce); a matrix
    // whose segment is not 16-byte aligned takes the scalar path
    p->out_off.assign(num_tensors, 0);
    for (int t = 0; t < num_tensors; ++t) {
        int64_t numel = 1;
        for (int64_t x : p->shapes[t]) numel *= x;
        p->out_off[t] = p->out_total;
        p->out_total += numel;
    }
    int64_t poff = 0, qoff = 0;
    for (size_t gi = 0; gi < p->groups.size(); ++gi) {
        auto& g = p->groups[gi];
        g.poff = poff;
        g.qoff = qoff;
        for (size_t b = 0; b < g.tensors.size(); ++b) {
            MatDesc md{};
            md.n = g.n;
            md.m = g.m;
            md.r = g.r;
            md.poff = poff + int64_t(b) * g.n * g.r;
            md.qoff = qoff + int64_t(b) * g.m * g.r;
            md.out_off = p->out_off[g.tensors[b]];
            md.tensor = g.tensors[b];
            md.group = int(gi);
            p->mats.push_back(md);
            // rank buckets 16 / 32: k_even's and k_apply's instances know the scalar (V = 1) layout
            // alone, for every matrix of the plan, also one whose own rank is capped at 8 or less by
            // its rows or columns (a [3, 200] matrix: with the vector layout its even product and
            // apply tiles covered a quarter of each strip and the rest was never written)
            const bool bucket_vec = p->rbucket <= 8 || p->rbucket > 32;
            p->base_vec.push_back(
                (dtype != PSGD_F64 && g.m % 4 == 0 && g.r <= 8 && bucket_vec && md.out_off % 4 == 0) ? 1 : 0);
        }
        poff += int64_t(g.tensors.size()) * g.n * g.r;
        qoff += int64_t(g.tensors.size()) * g.m * g.r;
        // orthonormalisation units (reference orthogonalize() is called per group batch, :188)
        if (g.r == 1) {
            p->units_p.push_back(OrthUnit{g.poff, g.n, 1, int32_t(g.tensors.size())});
            p->units_q.push_back(OrthUnit{g.qoff, g.m, 1, int32_t(g.tensors.size())});
            p->unit_group_p.push_back(int32_t(gi));
            p->unit_group_q.push_back(int32_t(gi));
        } else {
            for (size_t b = 0; b < g.tensors.size(); ++b) {
                p->units_p.push_back(OrthUnit{g.poff + int64_t(b) * g.n * g.r, g.n, g.r, 1});
                p->units_q.push_back(OrthUnit{g.qoff + int64_t(b) * g.m * g.r, g.m, g.r, 1});
                p->unit_group_p.push_back(int32_t(gi));
                p->unit_group_q.push_back(int32_t(gi));
            }
            p->panel_p = std::max(p->panel_p, g.n);  // longest rank>1 panel (rows)
            p->panel_q = std::max(p->panel_q, g.m);
        }
    }
    p->ptot = poff;
    p->qtot = qoff;
    p->fmax = std::max(poff, qoff);
    // folded orthonormalisation (projection form): every Q unit one panel of rbucket columns
    p->qfold_ok = !p->f64() && (p->rbucket == 2 || p->rbucket == 4) && !p->units_q.empty() &&
                  env_int("PSGD_QFOLD", 1) != 0;
    for (const OrthUnit& u : p->units_q) p->qfold_ok = p->qfold_ok && u.r == p->rbucket && u.count == 1;
    p->layout(num_tensors);
    *out_plan = p.release();
    return PSGD_OK;
}

int psgd_plan_destroy(psgd_plan* plan) {
    delete plan;
    return PSGD_OK;
}

int psgd_plan_num_groups(const psgd_plan* p, int32_t* out) {
    if (!p || !out) return fail(PSGD_ERR_VALUE, "null argument");
    *out = int32_t(p->groups.size());
    return PSGD_OK;
}

int psgd_plan_group(const psgd_plan* p, int32_t g, int64_t* n, int64_t* m, int32_t* r, int32_t* count) {
    if (!p || g < 0 || g >= int32_t(p->groups.size())) return fail(PSGD_ERR_VALUE, "group index out of range");
    const auto& gr = p->groups[g];
    if (n) *n = gr.n;
    if (m) *m = gr.m;
    if (r) *r = gr.r;
    if (count) *count = int32_t(gr.tensors.size());
    return PSGD_OK;
}

int psgd_plan_factor_numel(const psgd_plan* p, int64_t* pn, int64_t* qn) {
    if (!p) return fail(PSGD_ERR_VALUE, "null plan");
    if (pn) *pn = p->ptot;
    if (qn) *qn = p->qtot;
    return PSGD_OK;
}

int psgd_plan_output_offset(const psgd_plan* p, int32_t i, int64_t* off) {
    if (!p || !off || i < 0 || i >= int32_t(p->out_off.size())) return fail(PSGD_ERR_VALUE, "tensor index out of range");
    *off = p->out_off[i];
    return PSGD_OK;
}

int psgd_plan_output_numel(const psgd_plan* p, int64_t* numel) {
    if (!p || !numel) return fail(PSGD_ERR_VALUE, "null argument");
    *numel = p->out_total;
    return PSGD_OK;
}

int psgd_plan_workspace_bytes(const psgd_plan* p, int64_t* bytes) {
    if (!p || !bytes) return fail(PSGD_ERR_VALUE, "null argument");
    *bytes = int64_t(p->ws_bytes);
    return PSGD_OK;
}

int psgd_plan_compression_rate(const psgd_plan* p, double* rate, double* unc, double* comp) {
    if (!p) return fail(PSGD_ERR_VALUE, "null plan");
    if (rate) *rate = p->unc_floats / p->comp_floats;
    if (unc) *unc = p->unc_floats;
    if (comp) *comp = p->comp_floats;
    return PSGD_OK;
}

int psgd_plan_bind(psgd_plan* p, int32_t device, void* P, void* Q, void* workspace) {
    if (!p || !P || !Q || !workspace) return fail(PSGD_ERR_VALUE, "null argument");
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(PSGD_ERR_LAYOUT, "workspace must be 16-byte aligned");
    DevScope scope(device);
    p->device = device;
    p->P = static_cast<float*>(P);  // fp64 plans: double buffers (see P64/Q64)
    p->Q = static_cast<float*>(Q);
    p->ws = static_cast<char*>(workspace);
    p->norm_rec.have = false;  // a recorded term set names the buffers of the previous binding
    const size_t nt = p->shapes.size();
    p->grad_tab.bind(p->dev<char>(p->o_ptrs), nt);
    p->rdst_tab.bind(p->dev<char>(p->o_rdst), nt);
    p->odst_tab.bind(p->dev<char>(p->o_odst), nt);
    if (int st = p->upload_tiles()) return st;
    // the lists no re-tiling rebuilds (the fp64 ones are empty for the other plans)
    if (int st = upload_all(p->ws, p->units_p, p->units_q, p->munits_p, p->munits_q, p->f64_even, p->f64_odd,
                            p->f64_apply, p->f64_part_off))
        return st;
    if (p->wide())  // (their lists are carved for wide plans only)
        if (int st = upload_all(p->ws, p->wide_even, p->wide_odd, p->wide_apply, p->wide_gp, p->wide_gq, p->wide_slot_p,
                                p->wide_slot_q))
            return st;
    PSGD_HIP(hipMemset(p->ws + p->o_ss0, 0, size_t(std::max<int64_t>(p->ss0_cap, 1)) * sizeof(float)));
    p->bound = true;
    return PSGD_OK;
}

int psgd_out_factor(const psgd_plan* p, int64_t step, int32_t it, int32_t* which) {
    if (!p || !which) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0 || it < 0 || it >= p->iters) return fail(PSGD_ERR_VALUE, "step/iteration out of range");
    *which = p->even(step, it) ? 0 : 1;
    return PSGD_OK;
}

// ------------------------------------------------------------- buckets (W > 1) ---
int psgd_plan_set_buckets(psgd_plan* p, int32_t nbuckets, const int32_t* group_end) {
    if (!p) return fail(PSGD_ERR_VALUE, "null plan");
    if (nbuckets < 0 || (nbuckets > 0 && !group_end)) return fail(PSGD_ERR_VALUE, "bad bucket list");
    const int32_t ng = int32_t(p->groups.size());
    int32_t prev = 0;
    for (int b = 0; b < nbuckets; ++b) {
        if (group_end[b] <= prev || group_end[b] > ng) return fail(PSGD_ERR_VALUE, "bucket group ends must increase");
        prev = group_end[b];
    }
    if (nbuckets > 0 && prev != ng) return fail(PSGD_ERR_VALUE, "the last bucket must end at the last group");
    if (nbuckets > kMaxBuckets) return fail(PSGD_ERR_VALUE, "at most 8 buckets");
    if (p->wide()) {
        if (nbuckets > 1) return fail(PSGD_ERR_VALUE, "buckets are not supported for ranks above 32");
        return PSGD_OK;  // one bucket is the whole plan: nothing to re-tile
    }
    DevScope scope(p->device);
    if (p->bound) PSGD_HIP(hipDeviceSynchronize());  // the tile tables are rewritten below
    p->bucket_gend.assign(group_end, group_end + nbuckets);
    p->spans.clear();
    if (!p->f64()) {
        p->set_vec(p->vec_now);  // per-bucket segmentation of the even product, spans
        if (p->bound)
            if (int st = p->upload_tiles()) return st;
    }
    return PSGD_OK;
}

int psgd_plan_bucket_range(const psgd_plan* p, int32_t b, int64_t* p_off, int64_t* p_len, int64_t* q_off,
                           int64_t* q_len) {
    if (!p || b < 0 || b >= int32_t(std::max<size_t>(p->spans.size(), 1))) return fail(PSGD_ERR_VALUE, "bucket out of range");
    const psgd_plan::Span sp = p->spans.empty() ? p->full_span() : p->spans[b];
    if (p_off) *p_off = sp.p[0];
    if (p_len) *p_len = sp.p[1] - sp.p[0];
    if (q_off) *q_off = sp.q[0];
    if (q_len) *q_len = sp.q[1] - sp.q[0];
    return PSGD_OK;
}

int psgd_plan_fused_final(const psgd_plan* p, int64_t step, int32_t aggregate, int32_t* fused) {
    if (!p || !fused) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0) return fail(PSGD_ERR_VALUE, "step out of range");
    StepCtx c;
    c.fuse = c.write_out = aggregate != 0;
    const IterRoute r = p->route(step, p->iters - 1, c);
    *fused = r.pass != IterRoute::PassFinal ? 0 : r.proj ? 2 : 1;
    return PSGD_OK;
}

int psgd_plan_is_wide(const psgd_plan* p, int32_t* out) {
    if (!p || !out) return fail(PSGD_ERR_VALUE, "null argument");
    *out = p->wide() ? 1 : 0;
    return PSGD_OK;
}

int psgd_plan_odd_even(const psgd_plan* p, int64_t step, int32_t it, int32_t* on) {
    if (!p || !on) return fail(PSGD_ERR_VALUE, "null argument");
    if (step < 0 || it < 0 || it >= p->iters) return fail(PSGD_ERR_VALUE, "step/iteration out of range");
    *on = p->route(step, it, world1_ctx(StepCtx{})).pass == IterRoute::PassOddEven ? 1 : 0;  // psgd_aggregate's step
    return PSGD_OK;
}

// ------------------------------------------------------------- benchmark timing ---
int psgd_plan_set_timing(psgd_plan* p, int32_t enable) {
    if (!p) return fail(PSGD_ERR_VALUE, "null plan");
    p->timing = enable != 0;
    p->ev_used = 0;
    return PSGD_OK;
}

int psgd_plan_timing_read(psgd_plan* p, double* total_ms, int32_t* launches) {
    if (!p || !total_ms || !launches) return fail(PSGD_ERR_VALUE, "null argument");
    DevScope scope(p->device);
    double sum = 0.0;
    for (size_t i = 0; i < p->ev_used; ++i) {
        PSGD_HIP(hipEventSynchronize(p->ev_pool[i].second));
        float ms = 0.f;
        PSGD_HIP(hipEventElapsedTime(&ms, p->ev_pool[i].first, p->ev_pool[i].second));
        sum += ms;
    }
    *total_ms = sum;
    *launches = int32_t(p->ev_used);
    p->ev_used = 0;
    return PSGD_OK;
}

}  // extern "C"
