// Host-side definitions shared by the units behind the C ABI of include/psgd.h:
//   psgd_geometry.cpp  tile geometry, segmentation, work-list capacities and the workspace carve
//   psgd_plan.cpp      plan lifecycle: create, queries, bind, buckets, timing
//   psgd_step.cpp      step drivers (one stage function per IterRoute pass), the final-pass launch
//                      functions shared with admission, and the reducer building blocks
//   psgd_mixed.cpp     psgd_aggregate_mixed[_comm]: admission of the mixed instances, fold queries
//   psgd_direct.cpp    psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst: admission, state, entry points
//   psgd_norm.cpp      psgd_clip_outputs / psgd_plan_norm_form: form choice, state, launches
//   psgd_guard.cpp     psgd_guard_outputs: skipping a non-finite step (state, launches)
//   psgd_ipc.cpp       the IPC exchange arena and psgd_aggregate_ipc
//   psgd_flat.cpp      flat pack and DDP run tables
//   psgd_comm.cpp      the communicator behind psgd_aggregate_comm
// Here: the plan, the per-call StepCtx, and the step route (IterRoute / OutRoute, psgd_plan::route /
// out_route at the end of this file): the one place that decides what an iteration launches.
// No torch: plain pointers, hipStream_t as void*. Never included by device code.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "psgd.h"
#include "psgd_internal.h"

namespace psgd {

// per-dtype kernel launchers (psgd_*_f32.hip / psgd_*_bf16.hip) and their dtype dispatch
#define PSGD_PER_DTYPE(ret, fn, ...) \
    ret fn##_f32(__VA_ARGS__);       \
    ret fn##_bf16(__VA_ARGS__);
PSGD_PER_DTYPE(hipError_t, launch_even, int R, int nres, const ProductArgs& a, int nwg, hipStream_t s)
PSGD_PER_DTYPE(int, even_resident, int R)
PSGD_PER_DTYPE(hipError_t, launch_product_odd, int R, int nres, const ProductArgs& a, int ntiles, hipStream_t s)
PSGD_PER_DTYPE(hipError_t, launch_apply, int R, int nterms, bool shared, const ApplyArgs& a, int ntiles, hipStream_t s)
PSGD_PER_DTYPE(hipError_t, launch_odd_mfma, int R, int nres, const ProductArgs& a, int ntiles, hipStream_t s)
PSGD_PER_DTYPE(hipError_t, launch_final_odd, int R, int nres, int smax, const FinalArgs& a, int ntiles, hipStream_t s,
               int* waves)
PSGD_PER_DTYPE(hipError_t, launch_lowrank_out, int R, int nterms, const ApplyArgs& a, int ntiles, hipStream_t s)
PSGD_PER_DTYPE(hipError_t, launch_final_oe, int nres, int smax, const FinalArgs& a, int ntiles, hipStream_t s, int* waves)
#undef PSGD_PER_DTYPE
hipError_t launch_even(int dtype, int R, int nres, const ProductArgs& a, int nwg, hipStream_t s);
hipError_t launch_product_odd(int dtype, int R, int nres, const ProductArgs& a, int ntiles, hipStream_t s);

// records the message for psgd_last_error and returns `code`
int fail(int code, const std::string& msg);

#define PSGD_HIP(expr)                                                                   \
    do {                                                                                 \
        const hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess)                                                            \
            return fail(PSGD_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline int64_t pow2ceil(int64_t x) {
    int64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
int64_t env_int(const char* name, int64_t dflt);
int upload(void* dst, const void* src, size_t bytes);  // synchronous host-to-device copy

// One device work list: the host vector (the list is used as one), its capacity in elements and
// its byte offset in the caller's workspace. carve() places it once at create; every upload()
// checks the capacity, so a re-tiling of a bound plan can never write past the list's region.
template <typename T>
struct DevList : std::vector<T> {
    const char* name;
    size_t cap = 0, off = 0;
    explicit DevList(const char* n) : name(n) {}
    void carve(size_t& ws_off, size_t capacity) {
        off = ws_off;
        cap = capacity;
        ws_off = align256(ws_off + cap * sizeof(T));
    }
    T* dev(char* ws) const { return reinterpret_cast<T*>(ws + off); }
    int upload(char* ws) const {
        if (this->size() > cap)
            return fail(PSGD_ERR_STATE, std::string("work list ") + name + " exceeds its workspace capacity");
        return psgd::upload(ws + off, this->data(), this->size() * sizeof(T));
    }
};
template <typename... L>
int upload_all(char* ws, const L&... lists) {  // stops at the first failure
    int st = PSGD_OK;
    ((st = st ? st : lists.upload(ws)), ...);
    return st;
}

// Device-resident pointer tables (gradients, destinations) without a host synchronisation.
// kSlots tables live in the caller's workspace; a call whose pointer set matches a slot uses
// it as is (callers that rotate a few gradient sets, or get fresh tensors from the caching
// allocator, hit after the first round). A miss takes the least recently used slot and
// uploads into it with hipMemcpyAsync ON THE LAUNCH STREAM from a pinned staging copy, so
// the copy is ordered after every earlier launch on that stream that may still read the
// slot, and the host never waits (the reference hands tensors to torch ops, which never
// synchronise either). Calls of one plan must be ordered on one stream (as torch's are).
struct TableCache {
    static constexpr int kSlots = 4;
    size_t n = 0;              // pointers per table
    char* dev = nullptr;       // kSlots * n pointers inside the workspace
    std::vector<void*> host[kSlots];
    uint64_t stamp[kSlots] = {};
    uint64_t clock = 0;
    int cur = -1;
    void** pinned = nullptr;   // kSlots * n staging pointers (hipHostMalloc)
    hipEvent_t ev[kSlots] = {};
    bool live[kSlots] = {};

    static size_t bytes(size_t n) { return size_t(kSlots) * std::max<size_t>(n, 1) * sizeof(void*); }
    void bind(char* d, size_t count) {
        release();
        dev = d;
        n = count;
        for (auto& h : host) h.clear();
        cur = -1;
    }
    void release() {
        for (int i = 0; i < kSlots; ++i) {
            if (live[i]) (void)hipEventSynchronize(ev[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            ev[i] = nullptr;
            live[i] = false;
        }
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr;
    }
    ~TableCache() { release(); }
    bool match(int i, void* const* p) const { return host[i].size() == n && std::equal(p, p + n, host[i].begin()); }
    // 0 on success, else a hipError_t
    hipError_t select(void* const* p, hipStream_t s) {
        ++clock;
        if (cur >= 0 && match(cur, p)) {
            stamp[cur] = clock;
            return hipSuccess;
        }
        int victim = 0;
        for (int i = 0; i < kSlots; ++i) {
            if (match(i, p)) {
                cur = i;
                stamp[i] = clock;
                return hipSuccess;
            }
            if (stamp[i] < stamp[victim]) victim = i;
        }
        if (!pinned) {
            hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&pinned), bytes(n), hipHostMallocDefault);
            if (e != hipSuccess) {
                pinned = nullptr;
                return e;
            }
            for (int i = 0; i < kSlots; ++i)
                if ((e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess) return e;
        }
        // the staging slot may still feed the previous upload into this slot
        if (live[victim]) {
            const hipError_t e = hipEventSynchronize(ev[victim]);
            if (e != hipSuccess) return e;
        }
        void** stage = pinned + size_t(victim) * n;
        std::copy(p, p + n, stage);
        hipError_t e = hipMemcpyAsync(dev + size_t(victim) * n * sizeof(void*), stage, n * sizeof(void*),
                                      hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipEventRecord(ev[victim], s);
        if (e != hipSuccess) return e;
        live[victim] = true;
        host[victim].assign(p, p + n);
        stamp[victim] = clock;
        cur = victim;
        return hipSuccess;
    }
    void* const* table() const { return reinterpret_cast<void* const*>(dev + size_t(cur) * n * sizeof(void*)); }
};

struct DevScope {  // make `dev` current for the scope, restore afterwards
    int prev = -1;
    explicit DevScope(int dev) {
        (void)hipGetDevice(&prev);
        if (dev >= 0 && dev != prev) (void)hipSetDevice(dev);
    }
    ~DevScope() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

// Persistent even product (k_even): workgroups per launch (CUs x workgroups per CU), at least
// even_min gradient elements per workgroup (small plans use fewer, fuller workgroups), at
// most kMaxBuckets buckets (each bucket launch spreads over the whole chip).
constexpr int kCUs = 256;                // MI355X
constexpr int kEvenWpcMax = 16;          // k_even workgroups per CU (PSGD_EVEN_WPC cap)
constexpr int kEvenWgMax = kEvenWpcMax * kCUs;  // workgroups per launch (capacity)
constexpr int kMaxBuckets = 8;

int fin_bucket(int s);  // kernel instance (segments per row) serving s segments; 0: none

}  // namespace psgd

namespace psgd {
struct StepCtx;
struct IterRoute;
struct OutRoute;
}  // namespace psgd

using namespace psgd;  // the opaque C types below are global (include/psgd.h)

struct psgd_plan {
    int rank = 0, iters = 0, dtype = 0;
    std::vector<std::vector<int64_t>> shapes;
    struct Group {
        int64_t n, m;
        int r;
        std::vector<int> tensors;
        int64_t poff, qoff;
    };
    std::vector<Group> groups;
    DevList<MatDesc> mats{"mats"};  // group order
    std::vector<int> base_vec;  // vector path possible by shape (m % 4 == 0, r <= 8)
    std::vector<int> vec_now;   // currently active vector flags
    std::vector<int64_t> out_off;
    int64_t out_total = 0, ptot = 0, qtot = 0, fmax = 0;
    int rbucket = 1;
    int64_t tile_elems = 16384;
    DevList<Tile> tiles{"tiles"};        // lane-column tiles of every matrix (apply, low-rank output)
    DevList<Tile> tiles_ov{"tiles_ov"};  // lane-column tiles of the odd-VALU matrices
    DevList<Tile> tiles_om{"tiles_om"};  // MFMA tiles of the odd-MFMA matrices
    DevList<Tile> tiles_fin{"tiles_fin"};  // row blocks of the fused final odd pass
    // the K-term form's own row blocks when they differ from the projection form's (MatDesc::
    // fin_rows_kt); empty: the K-term form uses tiles_fin
    DevList<Tile> tiles_fin_kt{"tiles_fin_kt"};
    // per row block of tiles_fin / tiles_fin_kt / tiles_oe (same index) the sum-of-squares ranges
    // of its rank-1 prologue (FinRng); rebuilt with the reduction items (fill_seam_descriptors)
    DevList<FinRng> rng_fin{"rng_fin"}, rng_fin_kt{"rng_fin_kt"}, rng_oe{"rng_oe"};
    // (they serve the rank-1 norm folds: built, carved and uploaded for rank-1 fp32/bf16 plans only)
    bool seam_on() const { return rbucket == 1 && dtype != PSGD_F64; }
    // environment knobs, read once at create: PSGD_FUSE_FINAL, PSGD_FIN_PROJ, PSGD_OE (0: that
    // fused form is never used), PSGD_ORTH_CHOL (Cholesky-QR vs Householder)
    bool fuse_final_on = true, fin_proj_on = true, oe_on = true, orth_chol = true;
    bool mix_ingest_on = true;   // PSGD_MIXED_INGEST (0: psgd_aggregate_mixed never takes the ingest fold; A/B runs)
    bool fin_ok = false;         // every matrix fits the fused final odd pass (K-term form)
    bool fin_proj = false;       // ... in its projection form (I = 2, psgd_aggregate only)
    int fin_smax = 0;
    int64_t fin_elems = 32768, fin_elems_kt = 32768;
    // output stores of the fused final pass nt only (psgd_stream.cuh kStAuxOutNt): plans whose
    // gradients exceed 32 MB; smaller plans keep the write-through policy
    int32_t out_nt = 0;
    // even product (k_even): segments, per-workgroup segment ranges (wg_seg[w] .. wg_seg[w+1]),
    // workgroups per CU and the minimum elements per workgroup (read at create)
    DevList<Seg> segs{"segs"};
    DevList<int32_t> wg_seg{"wg_seg"};
    int even_wpc = 4;
    int64_t even_segc = 4096;  // k_even cost model: elements-equivalent of one segment's fixed cost
    int64_t even_min = 16384;
    // odd-even pass (k_final_oe: rank 1, world size 1, I >= 3): an odd iteration followed by an
    // even one inside a step in ONE gradient pass; its partials (per K-term row block, [m]) are
    // summed by k_reduce over red_oe, the blocks' sums of P^2 (oe_ss) give the even iteration's
    // joint norm (grng_oe: per group its block range), and the items' sums of squares feed the
    // next fused iteration (grng_oe_items: per group its red_oe range)
    bool oe_ok = false;
    DevList<RedItem> red_oe{"red_oe"};
    DevList<Tile> tiles_oe{"tiles_oe"};  // its row blocks (MatDesc::oe_rows rows)
    DevList<int32_t> grng_oe{"grng_oe"}, grng_oe_items{"grng_oe_items"};
    int64_t oe_part_floats = 0;
    int32_t oe_blocks = 0;
    bool oe_at(int64_t step, int it, bool agg) const {  // iteration `it` runs the odd-even pass
        return oe_ok && agg && it >= 1 && it + 1 < iters && !even(step, it);
    }
    // reduction items (rebuilt with the geometry): even items follow the segmentation
    DevList<RedItem> red_even{"red_even"}, red_odd{"red_odd"};
    // per group: [begin, end) of its reduction items
    DevList<int32_t> grng_even{"grng_even"}, grng_odd{"grng_odd"};
    DevList<OrthUnit> units_p{"units_p"}, units_q{"units_q"};
    // one unit per MATRIX (paper-code Gram-Schmidt)
    DevList<OrthUnit> munits_p{"munits_p"}, munits_q{"munits_q"};
    TableCache grad_tab, rdst_tab, odst_tab;  // device pointer tables (gradients, destinations)
    int64_t panel_p = 0, panel_q = 0;
    int64_t part_odd_floats = 0;  // odd partials [odd strips][n][r] per matrix; even ones follow
    double unc_floats = 0, comp_floats = 0;
    // Scratch regions of the workspace that mirror no host list (byte offsets): the pointer
    // tables of the three TableCaches, factor history, product partials, sums of squares (two
    // parities of ss_stride floats; the iteration-0 fold's ss0_cap slots), the folded
    // orthonormalisation's Gram partials, R' of the last iteration's in-factor panels
    // (projection form, Q layout), the odd-even pass's partials and sums, the fp64 partials
    size_t o_ptrs = 0, o_rdst = 0, o_odst = 0, o_hist = 0, o_part = 0, o_ss = 0, ss_stride = 0, o_ss0 = 0,
           o_gram = 0, o_rq = 0, o_oe_part = 0, o_oe_ss = 0, o_f64_part = 0, ws_bytes = 0;
    int64_t ss0_cap = 0;
    // rank-1 iteration-0 norm fold: per strip-0 segment a sum-of-squares slot, and per group the
    // [begin, end) slot range
    DevList<int32_t> grng_ss0{"grng_ss0"};
    // Buckets of whole shape groups (W > 1 overlap, psgd_plan_set_buckets): per bucket the
    // [begin, end) range of every launch list (all are in matrix order) and of the P/Q buffers.
    struct Span {
        int32_t tiles[2], ov[2], om[2], fin[2], fin_kt[2], re[2], ro[2], up[2], uq[2], wg[2];
        int64_t p[2], q[2];
    };
    std::vector<int32_t> bucket_gend;              // exclusive group end per bucket
    std::vector<int32_t> bucket_wg;                // per bucket [begin, end) of its k_even workgroups
    std::vector<Span> spans;
    std::vector<int32_t> unit_group_p, unit_group_q;
    Span full_span() const;
    void build_spans();

    // fp64 plans (psgd_f64.hip): even tiles (64-column strip, 256-row chunk), odd tiles
    // (16-row blocks), apply tiles (row chunks of ~16k elements), even partial offsets
    DevList<Tile> f64_even{"f64_even"}, f64_odd{"f64_odd"}, f64_apply{"f64_apply"};
    DevList<int64_t> f64_part_off{"f64_part_off"};
    int64_t f64_part = 0;
    // wide plans (rank bucket 64 / 128, psgd_wide.hip): tiles of the even product, the odd
    // product and the apply pass (psgd_internal.h, WideArgs); the reduction items of both
    // parities live in red_even / red_odd; partials (floats) in their own region, carved and
    // uploaded for wide plans only
    DevList<Tile> wide_even{"wide_even"}, wide_odd{"wide_odd"}, wide_apply{"wide_apply"};
    int64_t wide_part = 0;
    size_t o_wide_part = 0;
    // their orthonormalisation (WideOrthArgs): per side (P units / Q units) the row-block items of
    // the panels and each unit's first Gram-partial slot; the partials (wide_slots R x R fp64
    // matrices), and per unit M = R^-1, the column signs and the chain's verdict
    DevList<Tile> wide_gp{"wide_gp"}, wide_gq{"wide_gq"};
    DevList<int32_t> wide_slot_p{"wide_slot_p"}, wide_slot_q{"wide_slot_q"};
    int64_t wide_slots = 0;
    size_t o_wide_gram = 0, o_wide_m = 0, o_wide_sg = 0, o_wide_ok = 0;
    bool bound = false;
    int device = -1;
    float* P = nullptr;
    float* Q = nullptr;
    char* ws = nullptr;
    // benchmark timing of the final pass: event pairs recorded on the launch stream
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    // one-shot IPC all-reduce (psgd_ipc_*, psgd_aggregate_ipc): this rank's exchange buffer
    // (flags header + 2 parities x iters slots), the peers' opened mappings and session nonces,
    // the slot size (floats: factor region, then the flat region)
    char* ipc_buf = nullptr;      // this session's region of the process's exchange arena
    int ipc_chunk = -1;           // the region: arena chunk, byte offset and size
    size_t ipc_off = 0, ipc_bytes = 0;
    DevList<void*> ipc_peer{"ipc_peer"};
    DevList<uint32_t> ipc_nonces{"ipc_nonces"};
    int ipc_world = 0, ipc_rank = -1;
    int64_t ipc_slot = 0, ipc_flat_off = 0, ipc_flat_cap = 0;
    uint32_t ipc_nonce = 0;  // this rank's exchange session (psgd_ipc_create)
    // sessions of psgd_ipc_create2 on a wide plan (ipc_x2): every exchange of a step takes two epochs,
    // 2 * (step + 1) - 1 (the reduce-scatter phase of a two-shot exchange) and 2 * (step + 1) (its
    // all-gather phase, and every one-shot exchange); ipc_mode: 0 one-shot, 1 two-shot, 2 auto.
    // Sessions of psgd_ipc_create: false, epoch step + 1.
    bool ipc_x2 = false;
    int32_t ipc_mode = 0;
    // the factor exchange of side 0 (P, odd iterations) / 1 (Q, even ones) of the open session runs
    // two-shot (psgd_ipc_two_shot; the driver decides from this)
    bool ipc_two_shot(int side) const {
        if (!ipc_x2 || ipc_world < 2 || ipc_mode == 0) return false;
        if (ipc_mode == 1) return true;
        return ipc_world >= 3 && (side ? qtot : ptot) * int64_t(sizeof(float)) >= kXchgTwoShotBytes;
    }
    // sticky timeout word of the exchange waits: pinned host memory mapped into the device
    // (k_xchg stores 1 with a system-scope store), so every psgd_aggregate_ipc call can check it
    // without synchronising; cleared only by psgd_ipc_close
    int32_t* xerr_host = nullptr;
    int32_t* xerr_dev = nullptr;
    bool xerr_set() const { return xerr_host && __atomic_load_n(xerr_host, __ATOMIC_ACQUIRE) != 0; }
    unsigned long long* stamp_buf = nullptr;  // diagnostic k_even stamps (PSGD_EVEN_STAMPS)
    size_t stamp_words = 0;
    // psgd_aggregate_mixed (psgd_mixed.cpp): state of its own, created by the first mixed call or
    // fold query of a bound plan; nothing of it lives in the caller's workspace (whose carve stays
    // as it is), the device side is one small allocation owned by the plan
    struct Mixed {
        // admission of the mixed instances for the plan's current tiling (`key`): at least two
        // waves per SIMD and no scratch, asked of the runtime like the fused final pass's
        uint64_t key = ~uint64_t(0);
        bool fin_in = false;       // single-pass k_final_odd_mix with the ingest fold
        bool out[2] = {};          // the final pass of even / odd steps stores bf16
        char* dev = nullptr;       // pointer tables of the bf16 gradients (TableCache slots)
        size_t unc_cap = 0;        // ... and of the uncompressed bf16 gradients (entries)
        char* unc_dev = nullptr;
        TableCache src_tab, unc_tab;
        psgd_runs* add = nullptr;  // the run-table ADD (k_runs_mix) of steps without an ingest fold
        char* add_ws = nullptr;
        // psgd_aggregate_mixed_comm: admission of the final pass's bf16-output instance per
        // communicator kind ([0]: world size > 1, [1]: a 1-rank communicator) and step parity, and
        // the fp32 staging of the flat tail around its collective (made or grown by the first
        // call that needs it, like unc_dev)
        uint64_t comm_key = ~uint64_t(0);
        bool comm_out[2][2] = {};
        float* stage = nullptr;
        size_t stage_cap = 0;      // floats
        // psgd_aggregate_mixed_comm_dst: admission of the destination-table instances (a key of
        // their own, indexed like comm_out), and the destinations' pointer tables, beside src_tab
        // in `dev` and beside unc_tab in `unc_dev` (DDP rebuilds its buckets once: the pointers
        // change after the first iteration and are stable from then on)
        uint64_t dst_key = ~uint64_t(0);
        bool dst_out[2][2] = {};
        TableCache dst, unc_dst;
    };
    Mixed* mixed = nullptr;
    // psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst (psgd_direct.cpp): state of its own like
    // Mixed, created by the first call or psgd_plan_dst_ok query; nothing of it lives in the
    // caller's workspace. Admission of the fp32 destination-table instances of the output pass
    // per communicator kind ([0]: world size > 1, [1]: one rank) and step parity under a key of
    // its own; the destinations' pointer tables (change-detected: DDP rebuilds its buckets once);
    // the fp32 staging of the flat tail (`flat->total` floats, grown by the first call that needs it)
    struct Direct {
        uint64_t key = ~uint64_t(0);
        bool ok[2][2] = {};
        char* dev = nullptr;
        TableCache dst, unc_dst;
        size_t unc_cap = 0;
        char* unc_dev = nullptr;
        float* stage = nullptr;
        size_t stage_cap = 0;  // floats
    };
    Direct* direct = nullptr;
    // psgd_clip_outputs (psgd_norm.cpp). The record: the term set the output pass of `step` read at
    // world size `world` (ApplyArgs::apx and alpha), written where that set is built
    // (decompress_impl; final_stage on steps whose fused final pass wrote the output) and
    // dropped when the next step's first iteration starts, so the norm entry never re-derives a
    // route. Bucket calls (a span) leave none. `norm`: device state of its own like Mixed and
    // Direct (work items, Gram partials, per-tensor squares, stream partials), made by the first
    // psgd_clip_outputs call; nothing of it lives in the caller's workspace.
    struct NormRec {
        bool have = false;
        int64_t step = -1;
        int32_t world = 0, nterms = 0;
        float alpha = 0.f;
        Terms apx{};
    };
    NormRec norm_rec;
    void record_terms(int64_t step, int32_t world, const Terms& apx, int nterms, float alpha) {
        norm_rec.have = true;
        norm_rec.step = step;
        norm_rec.world = world;
        norm_rec.nterms = nterms;
        norm_rec.alpha = alpha;
        norm_rec.apx = apx;
    }
    int norm_env = 0;  // PSGD_NORM_FORM, read at create: 0 auto, 1 factors, 2 stream (A/B runs)
    struct Norm;
    Norm* norm = nullptr;
    // psgd_guard_outputs (psgd_guard.cpp): device state of its own like Norm (the flag word, the
    // gradient tensors' work items, the gradient pointer tables), made by the first call
    struct Guard;
    Guard* guard = nullptr;
    int64_t xslot_off(int64_t step, int it) const {  // byte offset of a slot in every buffer
        return kXchgHeader + ((step & 1) * iters + it) * ipc_slot * int64_t(sizeof(float));
    }
    float* xslot(int64_t step, int it) const { return reinterpret_cast<float*>(ipc_buf + xslot_off(step, it)); }
    // folded orthonormalisation of the projection form's Q panels (k_orth_chain): every Q unit
    // a single panel of exactly rbucket in {2, 4} columns; per-item Gram partials and per-unit
    // item ranges
    bool qfold_ok = false;
    DevList<int32_t> uitems{"uitems"};
    std::vector<int32_t> red_even_b, red_even_e;
    DevList<int32_t> mrng_even{"mrng_even"};  // per matrix [begin, end) of its even reduction items
    bool qfold(int64_t step, bool agg) const { return qfold_ok && iters == 2 && proj_final(step, agg); }

    ~psgd_plan();

    float* hist(int which, int k) const {  // 0: X (orthonormal in-factor), 1: Y local, 2: Y reduced
        return reinterpret_cast<float*>(ws + o_hist) + (int64_t(which) * iters + k) * fmax;
    }
    double* hist64(int which, int k) const {  // the same history, fp64 plans
        return reinterpret_cast<double*>(ws + o_hist) + (int64_t(which) * iters + k) * fmax;
    }
    bool f64() const { return dtype == PSGD_F64; }
    bool wide() const { return rbucket > 32; }  // effective rank 33-128 (fp32 / bf16 only)
    template <typename T>
    T* dev(size_t off) const { return reinterpret_cast<T*>(ws + off); }
    template <typename T>
    T* dev(const DevList<T>& l) const { return l.dev(ws); }
    bool even(int64_t step, int it) const { return ((step * iters + it) % 2) == 0; }

    // psgd_geometry.cpp
    void set_f64_tiles();
    void set_wide_tiles();
    void build_reduction();
    void fill_seam_descriptors();  // the FinRng lists, from the range tables
    void set_vec(const std::vector<int>& vec);
    void build_oe();
    void layout(int num_tensors);  // capacities, first tiling, workspace carve (once, at create)
    int upload_tiles() const;      // every list set_vec / set_f64_tiles rebuilds

    // What a step launches (the step route, below psgd::StepCtx): the drivers, the admission of
    // the mixed instances and the plan queries all read these two; nothing else decides a launch
    IterRoute route(int64_t step, int it, const StepCtx& c) const;
    OutRoute out_route(int64_t step, int world, const StepCtx& c) const;

    // The vocabulary route() / out_route() are written in (psgd_geometry.cpp sets the flags):
    // the last iteration of `step` runs fused (odd, and every matrix fits); `agg`: the caller
    // is psgd_aggregate (world size 1, output written), where the projection form also applies
    bool fused_final(int64_t step, bool agg) const { return (fin_ok || (agg && fin_proj)) && !even(step, iters - 1); }
    // the fused last iteration takes the projection form
    bool proj_final(int64_t step, bool agg) const { return agg && fin_proj && !even(step, iters - 1); }
    bool fused_final_at(int64_t step, int it, bool agg) const { return it == iters - 1 && fused_final(step, agg); }
    // Every group rank 1, iteration >= 1, a caller that folds (`fuse`: psgd_aggregate and the
    // IPC exchange): the joint-norm orthonormalisation of the in-factor is folded into the
    // neighbouring reductions (no orthonormalisation launch): the previous reduction leaves
    // per-item sums of squares, the product runs on the raw in-factor, and this iteration's
    // reduction divides by the norm and writes the normalised in-factor (reference
    // powersgd.py:186-188 + orthogonalization.py:5-6).
    bool fused_norm(bool fuse, int it) const { return fuse && rbucket == 1 && it >= 1; }
};

struct psgd_flat {
    int dtype = 0;
    DevList<FlatEntry> entries{"flat entries"};  // non-empty tensors only
    DevList<FlatItem> items{"flat items"};
    int32_t count = 0;
    int64_t total = 0;
    size_t o_ptrs = 0, ws_bytes = 0;
    bool bound = false;
    int device = -1;
    char* ws = nullptr;
    TableCache tab;  // device pointer tables of the tensors
};

// DDP bucket <-> parameter tensors (psgd_runs_*, include/psgd.h): the work items of one run
// table and the device pointer tables of the tensors it addresses
struct psgd_runs {
    int dtype = 0;         // the tensors' dtype
    int bucket_dtype = 0;  // the bucket side's (psgd_runs_create_mixed; else == dtype)
    int32_t ntensors = 0;
    DevList<RunItem> items{"run items"};
    int64_t bucket_numel = 0;  // one past the last bucket element any run touches
    size_t o_ptrs = 0, ws_bytes = 0;
    bool bound = false;
    int device = -1;
    char* ws = nullptr;
    TableCache tab;
    // source-table form: the bucket side is nsources separate tensors; per item its source index,
    // and the sources' device pointer tables (change-detected like the tensors')
    bool listed = false;
    int32_t nsources = 0;
    DevList<int32_t> item_src{"run item sources"};
    size_t o_src = 0;
    TableCache src_tab;
};

namespace psgd {

// What one call of a step driver passes down to compress_impl / decompress_impl: built on the
// entry point's stack, never stored in the plan.
struct StepCtx {
    bool fuse = false;       // fold the rank-1 joint norm into the kernels (psgd_plan::fused_norm)
    bool write_out = false;  // psgd_aggregate at world size 1: the fused final pass writes `out`
    const FlatArgs* fl = nullptr;            // uncompressed tensors riding in a launch
    const psgd_plan::Span* span = nullptr;   // one bucket's ranges; null: the whole plan
    void* out = nullptr;     // psgd_aggregate's output buffer (fused final pass)
    float* xout = nullptr;   // psgd_aggregate_ipc: this iteration's exchange slot
    // history slot of the RAW in-factor the rank-1 norm fold reads: 1 (the local reduction's
    // output, world size 1) or 2 (the exchange's summed copy, psgd_aggregate_ipc)
    int raw_slot = 1;
    // psgd_aggregate_ipc, ranks 2/4, two iterations: the exchange of iteration 0 left the summed
    // Q panels' Gram partials, so iteration 1 orthonormalises with k_orth_chain
    bool xgram = false;
    // psgd_aggregate_mixed: the final pass (and the flat items riding in it) runs its mixed
    // instance with these arguments; mix_in: the single-pass final kernel also ingests (ingest fold)
    const MixArgs* mix = nullptr;
    bool mix_in = false;
    // psgd_aggregate_mixed_comm_dst: the mixed output pass stores at these per-tensor destinations
    // (its destination-table instances) instead of `out`
    const MixDst* dst = nullptr;
    // psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst: the plan's own fp32 output pass stores at
    // these per-tensor destinations (psgd_apply_dst.hip) instead of `out`, and c.fl's items are
    // copy items from the staged flat tail
    const DirectDst* fdst = nullptr;
};

// The contexts of the two one-call steps, shared by the drivers and by admission (psgd_mixed.cpp):
// aggregate_ctx runs its iterations and output pass under world1_ctx(c); aggregate_comm_ctx its
// output pass under comm_out_ctx(mix) (its iterations under a plain StepCtx with the flat fold)
inline StepCtx world1_ctx(StepCtx c) {
    c.fuse = c.write_out = true;
    return c;
}
inline StepCtx comm_out_ctx(const MixArgs* mix, const MixDst* dst = nullptr) {
    StepCtx c;
    c.mix = mix;
    c.dst = dst;
    return c;
}

// The argument checks the step entry points of the C ABI share, in their order
inline int check_call(bool args, bool bound, bool range, const char* range_msg) {
    if (!args) return fail(PSGD_ERR_VALUE, "null argument");
    if (!bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (!range) return fail(PSGD_ERR_VALUE, range_msg);
    return PSGD_OK;
}
inline int check_out(const void* out) {
    if (reinterpret_cast<uintptr_t>(out) % 16) return fail(PSGD_ERR_LAYOUT, "output buffer must be 16-byte aligned");
    return PSGD_OK;
}
// ... and of a flat plan riding in a communicator step: `type_ok` with its own code and message
inline int check_flat(const psgd_flat* f, bool args, bool type_ok, int type_code, const char* type_msg) {
    if (!args) return fail(PSGD_ERR_VALUE, "null argument");
    if (!f->bound) return fail(PSGD_ERR_STATE, "flat plan is not bound");
    if (!type_ok) return fail(type_code, type_msg);
    return PSGD_OK;
}

// ------------------------------------------------------------------ step route ------
// What iteration `it` of `step` launches under a caller's StepCtx (fp32 / bf16 plans up to rank
// 32; fp64 and wide plans have no fused forms and one fixed sequence). Plain data from plan flags
// and the context: compress_impl launches what it says, admission (psgd_mixed.cpp) asks the
// runtime about the instances it names, the plan queries report it.
struct IterRoute {
    bool even;
    // the in-factor's orthonormalisation: folded into the neighbouring kernels (rank-1 joint norm),
    // a launch of its own (k_orth_*), or k_orth_chain on Gram partials left by the reduction /
    // the exchange
    enum Orth { OrthFolded, OrthLaunch, OrthChain } orth;
    // the gradient pass: k_even + k_reduce; k_product_odd / k_odd_mfma + k_reduce; k_final_oe (this
    // odd iteration and the next even product in one pass, no reduction); the fused last iteration
    // k_final_odd / k_final_proj; no product launch (k_reduce over the odd-even pass's partials)
    enum Pass { PassEven, PassOdd, PassOddEven, PassFinal, PassFromOddEven } pass;
    bool fused, fused0;        // rank-1 norm fold: in-factor from the previous reduction / iteration 0
    bool proj, own_kt;         // PassFinal: projection form; the K-term form on its own row blocks
    int final_nres;            // PassFinal: kFinProj or `it`
    bool ingest;               // PassFinal of psgd_aggregate_mixed: the single-pass ingest instance
    bool chain_from_exchange;  // OrthChain reads history slot 2 (the exchange's sum) instead of slot 1
    bool prev_after_oe;        // the in-factor's sums of squares / ranges were left after an odd-even pass
    bool ss_out, gram_out;     // what this iteration's reduction leaves for the next one
};

// The output pass after the iterations
struct OutRoute {
    enum Kind { None /* the fused last iteration wrote the output */, Lowrank, Apply } kind;
    enum Inst { Plain, Mix /* bf16 output, shared terms */, MixW /* bf16 output, two term sets */ } inst;
    bool shared;      // world size 1: the all-reduced factors are the local ones
    int32_t out_nt;   // output stores nt only (world size 1, large plans)
    bool timed;       // benchmark timing covers this launch
    bool flat;        // the context's flat items ride in the launch (k_lowrank_out takes none)
    bool dst;         // Mix / MixW / the mixed Lowrank: the destination-table instance (MixDst)
    bool fdst;        // Plain: the fp32 destination-table instance (DirectDst)
    int reduced_slot; // history slot of the earlier iterations' reduced factors (1: never copied to 2)
};

// psgd_step.cpp: the final pass of a route, for launching (the drivers) and for asking (admission:
// ntiles = 0, empty arguments, `*waves` receives the resident waves per SIMD of the instance that
// would run, 0 with scratch; only the fused and the mixed instances answer). `mix` null: the
// gradient type's own instance. launch_out_pass stamps the route's out_nt into `a`.
hipError_t launch_final_pass(const psgd_plan* p, const IterRoute& r, const FinalArgs& a, const MixArgs* mix, int ntiles,
                             hipStream_t s, int* waves);
hipError_t launch_out_pass(const psgd_plan* p, const OutRoute& o, ApplyArgs& a, const MixArgs* mix, int ntiles,
                           hipStream_t s, int* waves, const MixDst* dst = nullptr, const DirectDst* fdst = nullptr);

// psgd_step.cpp
int refresh_pointers(psgd_plan* p, void* const* grads, hipStream_t stream);
int compress_impl(psgd_plan* p, void* const* grads, int64_t step, int32_t it, hipStream_t s, StepCtx c);
int decompress_impl(psgd_plan* p, void* const* grads, void* out, int64_t step, int32_t world, hipStream_t s,
                    StepCtx c);
// psgd_flat.cpp: device-side arguments of a flat pack (selects or uploads the pointer table)
int flat_args(psgd_flat* f, void* const* tensors, void* flat, int32_t world, hipStream_t s, FlatArgs* out);
// psgd_ipc.cpp: the plan's exchange region goes back to the process's arena
void ipc_release(psgd_plan* p);
// psgd_ipc.cpp: what a step over the exchange needs of the session, checked before anything is
// launched: open, no timed-out wait pending, a 32-bit epoch
int ipc_check(const psgd_plan* p, int64_t step);
// psgd_ipc.cpp: the world-size-W step of psgd_aggregate_ipc; with `mix`, of psgd_aggregate_mixed_ipc
// (`grads` the fp32 residual, `out` / `flat_out` bf16, `unc` the uncompressed tensors' fp32
// residual); with `mix` and `dst`, of psgd_aggregate_mixed_ipc_dst (`out` and `flat_out` unused);
// with `fdst` alone, of psgd_aggregate_ipc_dst (`out` and `flat_out` unused: fdst->stage)
int aggregate_ipc_ctx(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f, void* const* unc,
                      void* flat_out, hipStream_t s, const MixArgs* mix, const MixDst* dst,
                      const DirectDst* fdst = nullptr);
// psgd_mixed.cpp: frees the plan's mixed state
void mixed_release(psgd_plan* p);
// psgd_direct.cpp: frees the plan's direct-store state
void direct_release(psgd_plan* p);
// psgd_direct.cpp, for psgd_clip_dst (psgd_norm.cpp): the plan is one the direct-store calls serve
// by shape (fp32, not wide, one bucket); and the device tables of `dst` / `unc_dst` (the slots the
// preceding direct-store call selected: no upload then) with the staged flat tail. A flat plan
// whose tail the plan has not staged (no preceding direct-store call with at least f->total
// floats): PSGD_ERR_STATE. Nothing is launched.
bool direct_shape_ok(const psgd_plan* p);
int direct_select(psgd_plan* p, void* const* dst, const psgd_flat* f, void* const* unc_dst, hipStream_t s, DirectDst* t);
// psgd_norm.cpp: frees the plan's norm state
void norm_release(psgd_plan* p);
// psgd_guard.cpp: frees the plan's guard state
void guard_release(psgd_plan* p);
// psgd_step.cpp: the world-size-1 step of psgd_aggregate / psgd_aggregate_flat under `c`
int aggregate_ctx(psgd_plan* p, void* const* grads, int64_t step, hipStream_t s, StepCtx c);
// psgd_step.cpp: the world-size-W step of psgd_aggregate_comm; with `mix`, of psgd_aggregate_mixed_comm;
// with `mix` and `dst`, of psgd_aggregate_mixed_comm_dst (`out` and `flat_out` unused); with `fdst`
// alone, of psgd_aggregate_comm_dst (`out` and `flat_out` unused: fdst->stage)
int aggregate_comm_ctx(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f, void* const* unc,
                       void* flat_out, psgd_comm* comm, hipStream_t s, const MixArgs* mix, const MixDst* dst = nullptr,
                       const DirectDst* fdst = nullptr);

}  // namespace psgd

inline IterRoute psgd_plan::route(int64_t step, int it, const StepCtx& c) const {
    IterRoute r{};
    r.even = even(step, it);
    r.fused = fused_norm(c.fuse, it);
    // rank 1, iteration 0, even: the joint norm of the (raw) state P is folded into the even
    // product (per-chunk sums of squares) and its reduction (divide, write normalised P)
    r.fused0 = rbucket == 1 && it == 0 && r.even && !fused_final_at(step, it, c.write_out);
    // projection form of the fused last iteration: its orthonormalisation leaves R' in o_rq
    r.proj = it == iters - 1 && proj_final(step, c.write_out);
    // folded orthonormalisation of the projection form: the even reduction leaves Gram partials
    // and k_orth_chain (no Gram pass, panel rows over several workgroups) replaces k_orth_chol
    const bool qf = qfold(step, c.write_out);
    r.chain_from_exchange = c.xgram && it == 1 && !r.even;  // the exchange left the summed Q's Gram
    r.orth = (qf && r.proj) || r.chain_from_exchange ? IterRoute::OrthChain
             : !r.fused && !r.fused0                 ? IterRoute::OrthLaunch
                                                     : IterRoute::OrthFolded;
    // after an odd-even pass the previous even reduction ran over its own item list
    r.prev_after_oe = !r.even && it >= 2 && oe_at(step, it - 2, c.write_out) && fused_norm(c.fuse, it - 2);
    if (r.fused && c.span == nullptr && oe_at(step, it, c.write_out))
        r.pass = IterRoute::PassOddEven;
    else if (fused_final_at(step, it, c.write_out))
        r.pass = IterRoute::PassFinal;
    else if (r.even && it >= 1 && c.span == nullptr && oe_at(step, it - 1, c.write_out) && fused_norm(c.fuse, it - 1))
        r.pass = IterRoute::PassFromOddEven;
    else
        r.pass = r.even ? IterRoute::PassEven : IterRoute::PassOdd;
    r.own_kt = !r.proj && !tiles_fin_kt.empty();
    r.final_nres = r.proj ? kFinProj : it;
    r.ingest = c.mix_in && it == 0;
    r.ss_out = fused_norm(c.fuse, it + 1) && it + 1 < iters;
    r.gram_out = qf && r.even && it + 2 == iters;  // the Q panels' Gram for k_orth_chain
    return r;
}

inline OutRoute psgd_plan::out_route(int64_t step, int world, const StepCtx& c) const {
    OutRoute o{};
    // after a fused last iteration the residual is written: output only, or (psgd_aggregate at
    // world size 1, which wrote the output too) nothing
    o.kind = !fused_final(step, c.write_out) ? OutRoute::Apply : c.write_out ? OutRoute::None : OutRoute::Lowrank;
    o.inst = !c.mix ? OutRoute::Plain : o.kind == OutRoute::Apply && world > 1 ? OutRoute::MixW : OutRoute::Mix;
    o.shared = world == 1;
    o.out_nt = world == 1 ? out_nt : 0;
    o.timed = o.kind == OutRoute::Apply;
    o.fdst = c.mix == nullptr && c.fdst != nullptr;
    o.flat = o.kind == OutRoute::Apply || c.mix != nullptr || o.fdst;
    o.dst = c.mix != nullptr && c.dst != nullptr;
    // fused (world size 1): the reduced factor was never copied to history slot 2
    o.reduced_slot = fused_norm(c.fuse, 1) ? 1 : 2;
    return o;
}
