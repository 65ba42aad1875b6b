// Flat pack of the uncompressed tensors (psgd_flat_*) and the DDP bucket <-> parameter run
// tables (psgd_runs_*) behind the C ABI of include/psgd.h.
#include <memory>

#include "psgd_plan.h"

// Device-side arguments of a flat pack (selects or uploads the pointer table, stream-ordered).
int psgd::flat_args(psgd_flat* f, void* const* tensors, void* flat, int32_t world, hipStream_t s, FlatArgs* out) {
    PSGD_HIP(f->tab.select(tensors, s));
    FlatArgs& a = *out;
    a = FlatArgs{};
    a.entries = f->entries.dev(f->ws);
    a.items = f->items.dev(f->ws);
    a.tensors = f->tab.table();
    a.flat = flat;
    a.nitems = int32_t(f->items.size());
    a.world = world;
    return PSGD_OK;
}

// One launch of a run table: `list` false, the single-bucket form on `bucket`; true, the
// source-table form on `sources`. mode: RunsMode (psgd_internal.h).
static int runs_launch(psgd_runs* r, bool list, const void* bucket, void* const* sources, void* const* tensors,
                       int mode, void* stream) {
    if (!r) return fail(PSGD_ERR_VALUE, "null argument");
    if (list != r->listed)
        return fail(PSGD_ERR_STATE, r->listed ? "run table has a source table: use psgd_runs_add_list / _gather_list"
                                              : "run table has no source table: use psgd_runs_add / _gather");
    if ((list ? !sources && r->nsources > 0 : !bucket && !r->items.empty()) || (!tensors && r->ntensors > 0))
        return fail(PSGD_ERR_VALUE, "null argument");
    if (!r->bound) return fail(PSGD_ERR_STATE, "run table is not bound");
    if (r->items.empty()) return PSGD_OK;
    DevScope scope(r->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    PSGD_HIP(r->tab.select(tensors, s));
    if (!list && r->bucket_dtype == r->dtype) {  // the tables of psgd_runs_create: k_runs
        RunsArgs a{};
        a.items = r->items.dev(r->ws);
        a.bucket = const_cast<void*>(bucket);
        a.tensors = r->tab.table();
        a.nitems = int32_t(r->items.size());
        PSGD_HIP(launch_runs(r->dtype, mode != kRunsGather, a, s));
        return PSGD_OK;
    }
    RunsMixArgs a{};
    a.items = r->items.dev(r->ws);
    a.tensors = r->tab.table();
    a.nitems = int32_t(r->items.size());
    if (list) {
        PSGD_HIP(r->src_tab.select(sources, s));
        a.src = r->item_src.dev(r->ws);
        a.sources = r->src_tab.table();
    } else {
        a.bucket = const_cast<void*>(bucket);
    }
    PSGD_HIP(launch_runs_mix(r->bucket_dtype, r->dtype, mode, a, s));
    return PSGD_OK;
}

static bool runs_dtype_ok(int32_t d) { return d == PSGD_F32 || d == PSGD_BF16 || d == PSGD_F64; }

// The table behind psgd_runs_create and psgd_runs_create_mixed (`source` null: one bucket).
static int runs_build(const int64_t* bucket_off, const int32_t* tensor, const int64_t* tensor_off, const int64_t* len,
                      const int32_t* source, int32_t nruns, int32_t ntensors, int32_t nsources, int32_t bucket_dtype,
                      int32_t dtype, psgd_runs** out) {
    std::unique_ptr<psgd_runs> r(new psgd_runs());
    r->dtype = dtype;
    r->bucket_dtype = bucket_dtype;
    r->ntensors = ntensors;
    r->listed = source != nullptr;
    r->nsources = r->listed ? nsources : 0;
    for (int32_t k = 0; k < nruns; ++k) {
        if (len[k] < 0 || bucket_off[k] < 0 || tensor_off[k] < 0 || tensor[k] < 0 || tensor[k] >= ntensors ||
            (source && (source[k] < 0 || source[k] >= nsources)))
            return fail(PSGD_ERR_VALUE, "run " + std::to_string(k) + " out of range");
        for (int64_t e = 0; e < len[k]; e += kRunItem) {
            r->items.push_back(RunItem{bucket_off[k] + e, tensor_off[k] + e, tensor[k],
                                       int32_t(std::min<int64_t>(kRunItem, len[k] - e))});
            if (source) r->item_src.push_back(source[k]);
        }
        r->bucket_numel = std::max(r->bucket_numel, bucket_off[k] + len[k]);
    }
    if (r->items.size() > size_t(INT32_MAX)) return fail(PSGD_ERR_VALUE, "run table too large for one launch");
    size_t off = align256(TableCache::bytes(size_t(std::max(ntensors, 1))));  // the pointer tables at o_ptrs = 0
    r->items.carve(off, std::max<size_t>(r->items.size(), 1));
    if (r->listed) {  // the sources' pointer tables and the items' source indices follow
        r->o_src = off;
        off = align256(off + TableCache::bytes(size_t(std::max(nsources, 1))));
        r->item_src.carve(off, std::max<size_t>(r->item_src.size(), 1));
    }
    r->ws_bytes = off;
    *out = r.release();
    return PSGD_OK;
}

extern "C" {

int psgd_flat_create(const int64_t* numels, int32_t count, int32_t dtype, psgd_flat** out) {
    if (!out) return fail(PSGD_ERR_VALUE, "null argument");
    *out = nullptr;
    if (count < 0 || (count > 0 && !numels)) return fail(PSGD_ERR_VALUE, "bad tensor list");
    if (dtype != PSGD_F32 && dtype != PSGD_BF16 && dtype != PSGD_F64)
        return fail(PSGD_ERR_DTYPE, "dtype must be fp32, bf16 or fp64");
    std::unique_ptr<psgd_flat> f(new psgd_flat());
    f->dtype = dtype;
    f->count = count;
    for (int i = 0; i < count; ++i) {
        if (numels[i] < 0) return fail(PSGD_ERR_VALUE, "negative numel");
        // empty tensors occupy no flat range: no lookup entry (their pointer slot stays)
        if (numels[i] > 0) f->entries.push_back(FlatEntry{f->total, numels[i], i, 0});
        f->total += numels[i];
    }
    for (size_t e = 0; e < f->entries.size(); ++e)
        for (int64_t st = 0; st < f->entries[e].numel; st += kFlatItem) f->items.push_back(FlatItem{int32_t(e), 0, st});
    size_t off = align256(TableCache::bytes(size_t(std::max(count, 1))));  // the pointer tables at o_ptrs = 0
    f->entries.carve(off, std::max<size_t>(f->entries.size(), 1));
    f->items.carve(off, std::max<size_t>(f->items.size(), 1));
    f->ws_bytes = off;
    *out = f.release();
    return PSGD_OK;
}

int psgd_flat_destroy(psgd_flat* f) {
    delete f;
    return PSGD_OK;
}

int psgd_flat_workspace_bytes(const psgd_flat* f, int64_t* bytes) {
    if (!f || !bytes) return fail(PSGD_ERR_VALUE, "null argument");
    *bytes = int64_t(f->ws_bytes);
    return PSGD_OK;
}

int psgd_flat_bind(psgd_flat* f, int32_t device, void* workspace) {
    if (!f || !workspace) return fail(PSGD_ERR_VALUE, "null argument");
    DevScope scope(device);
    f->device = device;
    f->ws = static_cast<char*>(workspace);
    f->tab.bind(f->ws + f->o_ptrs, size_t(f->count));
    if (int st = upload_all(f->ws, f->entries, f->items)) return st;
    f->bound = true;
    return PSGD_OK;
}

int psgd_flat_pack(psgd_flat* f, void* const* tensors, void* flat, int32_t world, void* stream) {
    if (!f || (!tensors && f->count > 0) || (!flat && f->total > 0)) return fail(PSGD_ERR_VALUE, "null argument");
    if (!f->bound) return fail(PSGD_ERR_STATE, "flat plan is not bound");
    if (world < 1) return fail(PSGD_ERR_VALUE, "world size must be >= 1");
    if (f->total == 0) return PSGD_OK;
    DevScope scope(f->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FlatArgs a;
    if (int st = flat_args(f, tensors, flat, world, s, &a)) return st;
    PSGD_HIP(launch_flat_pack(f->dtype, a, s));
    return PSGD_OK;
}

// ------------------------------------------------------ DDP run tables (psgd_runs) --
int psgd_runs_create(const int64_t* bucket_off, const int32_t* tensor, const int64_t* tensor_off,
                     const int64_t* len, int32_t nruns, int32_t ntensors, int32_t dtype, psgd_runs** out) {
    if (!out) return fail(PSGD_ERR_VALUE, "null argument");
    *out = nullptr;
    if (nruns < 0 || ntensors < 0 || (nruns > 0 && (!bucket_off || !tensor || !tensor_off || !len)))
        return fail(PSGD_ERR_VALUE, "bad run table");
    if (dtype != PSGD_F32 && dtype != PSGD_BF16 && dtype != PSGD_F64)
        return fail(PSGD_ERR_DTYPE, "dtype must be fp32, bf16 or fp64");
    return runs_build(bucket_off, tensor, tensor_off, len, nullptr, nruns, ntensors, 0, dtype, dtype, out);
}

int psgd_runs_create_mixed(const int64_t* bucket_off, const int32_t* tensor, const int64_t* tensor_off,
                           const int64_t* len, const int32_t* source, int32_t nruns, int32_t ntensors,
                           int32_t nsources, int32_t bucket_dtype, int32_t tensor_dtype, psgd_runs** out) {
    if (!out) return fail(PSGD_ERR_VALUE, "null argument");
    *out = nullptr;
    if (nruns < 0 || ntensors < 0 || nsources < 0 || (nruns > 0 && (!bucket_off || !tensor || !tensor_off || !len)))
        return fail(PSGD_ERR_VALUE, "bad run table");
    if (!runs_dtype_ok(bucket_dtype) || !runs_dtype_ok(tensor_dtype) ||
        (bucket_dtype != tensor_dtype && !(bucket_dtype == PSGD_BF16 && tensor_dtype == PSGD_F32)))
        return fail(PSGD_ERR_DTYPE, "bucket / tensor dtypes must be equal (fp32, bf16, fp64) or bf16 over fp32");
    return runs_build(bucket_off, tensor, tensor_off, len, source, nruns, ntensors, nsources, bucket_dtype,
                      tensor_dtype, out);
}

int psgd_runs_destroy(psgd_runs* r) {
    delete r;
    return PSGD_OK;
}

int psgd_runs_workspace_bytes(const psgd_runs* r, int64_t* bytes) {
    if (!r || !bytes) return fail(PSGD_ERR_VALUE, "null argument");
    *bytes = int64_t(r->ws_bytes);
    return PSGD_OK;
}

int psgd_runs_bind(psgd_runs* r, int32_t device, void* workspace) {
    if (!r || !workspace) return fail(PSGD_ERR_VALUE, "null argument");
    DevScope scope(device);
    r->device = device;
    r->ws = static_cast<char*>(workspace);
    r->tab.bind(r->ws + r->o_ptrs, size_t(r->ntensors));
    if (int st = r->items.upload(r->ws)) return st;
    if (r->listed) {
        r->src_tab.bind(r->ws + r->o_src, size_t(r->nsources));
        if (int st = r->item_src.upload(r->ws)) return st;
    }
    r->bound = true;
    return PSGD_OK;
}

int psgd_runs_add(psgd_runs* r, const void* bucket, void* const* tensors, void* stream) {
    return runs_launch(r, false, bucket, nullptr, tensors, kRunsAdd, stream);
}

int psgd_runs_gather(psgd_runs* r, void* bucket, void* const* tensors, void* stream) {
    return runs_launch(r, false, bucket, nullptr, tensors, kRunsGather, stream);
}

int psgd_runs_add_list(psgd_runs* r, void* const* sources, void* const* tensors, int32_t zero_source,
                       void* stream) {
    return runs_launch(r, true, nullptr, sources, tensors, zero_source ? kRunsAddZero : kRunsAdd, stream);
}

int psgd_runs_gather_list(psgd_runs* r, void* const* sources, void* const* tensors, void* stream) {
    return runs_launch(r, true, nullptr, sources, tensors, kRunsGather, stream);
}

}  // extern "C"
