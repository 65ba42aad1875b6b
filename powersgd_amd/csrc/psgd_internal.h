// Internal layout shared by the host units (psgd_plan.h) and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <stdint.h>

struct psgd_comm;  // include/psgd.h (psgd_comm.cpp)

namespace psgd {

// host side of the RCCL communicator (psgd_comm.cpp): the error message goes to
// psgd_last_error (comm_fail, psgd_plan.cpp); comm_allreduce = a grouped in-place SUM of one or
// two fp32 buffers, stream-ordered on s
int comm_fail(int code, const char* msg);
int comm_world(const psgd_comm* c);
int comm_allreduce(psgd_comm* c, float* buf, size_t n, float* buf2, size_t n2, hipStream_t s);
void comm_poison(psgd_comm* c, const char* why);  // every later comm_allreduce fails (PSGD_ERR_STATE)
bool comm_poisoned(const psgd_comm* c, std::string* why);  // checked before a step launches anything

// Benchmark timing of the final pass (psgd_plan_set_timing): while set, the final-pass launch
// records these events from its own dispatch packet (hipExtLaunchKernel), so the measured span
// is the kernel alone, without the marker packets of separate hipEventRecord calls.
struct KernelTiming {
    hipEvent_t start, stop;
};
extern thread_local const KernelTiming* g_kernel_timing;

constexpr int kMaxTerms = 16;   // == PSGD_MAX_ITERS
constexpr int kBlock = 256;     // threads per workgroup for the streaming kernels
constexpr int kWaves = kBlock / 64;

// One compressed matrix (the [n, m] view of a tensor). Stored in GROUP order, so the
// P/Q offsets below are monotone and reproduce the reference's _ps/_qs_buffer layout.
struct MatDesc {
    int64_t n, m;
    int64_t poff, qoff;     // offsets (floats) of this matrix's P [n,r] / Q [m,r] panels
    int64_t out_off;        // element offset in the flat output buffer
    int64_t part_even;      // column partials [nchunk][m][r] (even iterations)
    int64_t part_odd;       // row partials    [nstrip][n][r] (odd iterations)
    int32_t r;
    int32_t tensor;         // index into the gradient pointer table
    int32_t group;
    int32_t vec;            // 1: 4-element vector loads/stores (m % 4 == 0, aligned)
    int32_t lanes;          // L: lanes sharing one row inside a wave (power of two <= 64)
    int32_t nstrip;         // column strips of L*V columns
    int32_t nchunk;         // row chunks
    int32_t chunk_rows;     // rows per chunk (multiple of the block's rows per pass)
    // odd iterations (P = G Q): MFMA tiles when odd_mfma, else the lane-column tiles above
    int32_t odd_mfma;
    int32_t odd_nstrip;     // column strips of the odd partials (reduce pass)
    int32_t odd_sw;         // MFMA strip width (columns, multiple of 16)
    int32_t odd_chunk_rows; // MFMA chunk rows (multiple of 16 * kWaves)
    // fused final odd iteration (k_final_odd): a row group of fin_T threads owns a row
    // (fin_S segments of 4*fin_T columns); a workgroup covers fin_rows rows in the projection
    // form, fin_rows_kt in the K-term form
    int32_t fin_T;
    int32_t fin_S;
    int32_t fin_rows;
    int32_t fin_rows_kt;
    // odd-even pass (k_final_oe, rank 1, world size 1): row block b (oe_rows rows, the K-term
    // row-group geometry) leaves its partial of the next even product at oe_part + b * m and its
    // sum of P^2 at oe_ss[oe_blk0 + b]
    int64_t oe_part;
    int32_t oe_blk0;
    int32_t oe_rows;
};

// Streaming tile: rows [chunk*chunk_rows, +chunk_rows) x columns of one strip.
struct Tile {
    int32_t mat, strip, chunk;
    int32_t tensor;  // fp32/bf16 streaming tiles: the matrix's gradient-table index (its pointer
                     // load goes out beside the MatDesc load instead of after it)
};

// Even-product work unit of the persistent k_even (psgd_even.cuh): rows [row0, row1) of one
// column strip (L lanes x V columns) of one matrix. Workgroup w walks segments
// [wg_seg[w], wg_seg[w + 1]) in order; segment boundaries split the plan (or a bucket of it)
// into equal gradient byte ranges, one per workgroup, so a strip is cut only where a
// workgroup's range ends: its column partials are few (one per segment, not one per small tile).
// The matrix fields the pass needs are copied in, so a segment start is one descriptor load
// and one gradient-pointer load (no MatDesc round trip in between).
struct Seg {
    int64_t m;           // columns of the matrix
    int64_t poff, qoff;  // its P / Q panel offsets (floats)
    int64_t part;        // float offset of this segment's partials [strip columns][r] in the workspace
    int32_t row0, row1, strip;
    int32_t tensor;      // gradient-table index of the matrix
    int32_t ss;          // rank-1 norm fold: sum-of-squares slot of a strip-0 segment, else -1
    int32_t r, lanes;
    int32_t vec;         // 0: scalar columns; 1: 4-column vectors; 2: full-width strip fast path
                         // (64 lanes x 4 columns, r == the plan's rank bucket, < 2^31 bytes)
};

// Reduction item for the partial-sum pass: up to 64 * per consecutive factor elements of one
// matrix that share their partial layout: partial k of element start + j lies at
// pbase + k * pstride + j (even: one column strip's segments; odd: the matrix's strips).
constexpr int kRedElems = 64;  // fp64 plans: factor elements per reduction item (one per lane)
constexpr int kRedItem = 256;  // fp32/bf16 plans: at most this many factor elements per reduction item
constexpr int kRedWide = 64;   // ... when an element has at most this many partials (else 64)

struct RedItem {
    int32_t mat, start;
    int32_t per;     // fp32/bf16 plans: elements per lane (4: 256-element item; 1: 64 elements,
                     // for factors with many partials, where 4 per lane is one CU's bandwidth)
    int32_t cnt;     // elements in the item (<= 64 * per)
    int64_t pbase;   // partial 0 of element `start` (floats from the partial workspace)
    int32_t pstride; // floats between consecutive partials of one element
    int32_t np;      // partials per element
};

// Rank-1 plans, beside each row block of the fused final passes (tiles_fin, tiles_fin_kt,
// tiles_oe; same index): the sum-of-squares ranges its prologue sums, copied in from the
// per-group and per-matrix range tables as Seg copies the matrix fields for k_even, so their
// loads hang on the block index alone (no MatDesc and range-table round trips before them).
struct alignas(16) FinRng {
    int32_t g[2][2];  // the group's sums of squares [begin, end): [0] in the even reduction's
                      // items (grng_even), [1] in the items after an odd-even pass (grng_oe_items)
    int32_t mb, me;   // the matrix's even reduction items (rank-1 projection form: c)
    int32_t pad[2];
};
static_assert(sizeof(FinRng) == 32, "FinRng: two 16-byte vectors");

// Orthonormalisation unit: rank 1 -> one shape GROUP (joint norm over count*k values);
// rank > 1 -> one matrix (Householder QR of a k x r panel).
struct OrthUnit {
    int64_t off;    // offset (floats) in the P- or Q-layout buffer
    int64_t k;      // rows of each panel
    int32_t r;
    int32_t count;  // panels in the unit (group size for rank 1, 1 otherwise)
};

// A list of rank-r terms  P_k Q_k^T : P-layout [n,r] and Q-layout [m,r] panel buffers.
struct Terms {
    const float* p[kMaxTerms];
    const float* q[kMaxTerms];
};

struct FlatEntry {
    int64_t off, numel;  // dense offset in the flat buffer (non-empty tensors only)
    int64_t tensor;      // index into the pointer table
    int64_t pad;
};

// Flat-pack work item: kFlatItem consecutive elements of one entry.
constexpr int kFlatItem = 8 * kBlock;
struct FlatItem {
    int32_t entry, pad;
    int64_t start;
};

struct FlatArgs {
    const FlatEntry* entries;
    const FlatItem* items;
    void* const* tensors;
    void* flat;
    int32_t nitems;
    int32_t world;
};

struct ProductArgs {
    const MatDesc* mats;
    const Tile* tiles;
    void* const* grads;
    const float* x;      // orthonormal in-factor: P-layout (even) / Q-layout (odd)
    float* part;         // partial-sum workspace
    Terms res;           // error-feedback terms applied on the fly
    int32_t nres;
    // rank-1 iteration 0 with the norm folded (even product on the RAW state P): strip-0
    // segments write sum_rows P^2 of their rows to ss0[seg.ss]
    float* ss0;
    // even product (k_even): segments and per-workgroup [begin, end) (wg_seg[blockIdx],
    // wg_seg[blockIdx + 1]) of its nwg workgroups; workgroups nwg .. nwg + flat.nitems - 1 pack
    // the uncompressed tensors (world size > 1: the first iteration's launch carries them)
    const Seg* segs;
    const int32_t* wg_seg;
    int32_t nwg;
    FlatArgs flat;
    // diagnostic builds only (-DPSGD_EVEN_STAMPS, tools/even_stamps.py): per workgroup of k_even
    // kEvenStamps 64-bit words (s_memrealtime at entry and after each segment, the XCC / HW ids)
    unsigned long long* stamps;
};
constexpr int kEvenStamps = 8;

struct ApplyArgs {
    const MatDesc* mats;
    const Tile* tiles;
    void* const* grads;  // in: G_0, out: residual
    void* out;           // flat output buffer
    Terms res;           // local terms (residual)
    Terms apx;           // all-reduced terms (approximation), scaled by alpha
    int32_t nterms;
    float alpha;         // 1 / world_size
    // blocks [0, flat.nitems) pack the uncompressed tensors (AllReduce at world size 1)
    // inside the same launch; the ntiles tiles follow
    int32_t ntiles;
    FlatArgs flat;
    // optional destination tables (device arrays of per-tensor pointers): the residual goes
    // to rdst[i] instead of back into grads[i], the output to odst[i] instead of the flat
    // buffer (psgd_reconstruct)
    void* const* rdst;
    void* const* odst;
    int32_t out_nt;      // world size 1 (shared terms): output stores nt only (large plans, as the
                         // fused final pass's FinalArgs::out_nt), a separate kernel instance
};

struct ReduceArgs {
    const MatDesc* mats;
    const RedItem* items;
    const float* part;
    float* yloc;         // history copy of the local factor
    float* state;        // reference-visible state buffer (the out-factor)
    int32_t even;
    int32_t nmain;       // items[0, nmain) reduce the out-factor
    // Rank-1 fused normalisation (world size 1, iteration >= 1): the product ran on the RAW
    // in-factor `raw` (the previous iteration's reduced out-factor); its group norm comes
    // from the previous reduction's sum-of-squares partials `ss_in` (per item, group g's
    // items are grng_in[g] = [begin, end)). The reduction divides by it, and the extra
    // items nitems[0, nnorm) write the normalised in-factor to `xstate` and `hx`.
    const float* ss_in;
    const int32_t* grng_in;
    const RedItem* nitems;
    int32_t nnorm;
    const float* raw;
    float* xstate;
    float* hx;
    float* ss_out;       // per-item sum of squares of this reduction's output (or null)
    // Folded orthonormalisation (projection form, k_orth_chain): per item the upper Gram of
    // its output rows (kGramStride fp64 entries, rank gram_r in {2, 4}), or null
    double* gram;
    int32_t gram_r;
    float* xout;         // one-shot exchange (psgd_aggregate_ipc): the local factor also goes to
                         // this rank's exchange slot (same offsets as `state`), or null
};

constexpr int kGramStride = 10;  // fp64 Gram entries per reduction item (rank <= 4)

// k_orth_chain: Cholesky-QR of each Q panel from the reduction's Gram partials (no Gram pass
// over the panel), the panel rows split over several workgroups that each run the r x r chain
// and apply X = raw M to their slice. Fallback panels (ill-conditioned, unreflected columns):
// the slice-0 workgroup runs the exact Householder recursion on the whole panel.
struct ChainArgs {
    const OrthUnit* units;
    const int32_t* uitems;  // per unit: [begin, end) of its reduction items
    const double* gram;     // kGramStride per item
    const float* raw;       // Q layout: the reduced (raw) factor
    float* state;           // Q state: X
    float* hx;              // X history
    float* rfac;            // Q layout: R' (r x r) at each unit's offset
};

// Fused LAST iteration when it is odd (P = G_k X): a row group holds whole rows in
// registers, so the reduction over columns completes inside the workgroup and the same
// registers produce the residual (and, at world size 1, the output) without re-reading G.
struct FinalArgs {
    const MatDesc* mats;
    const Tile* tiles;    // (mat, 0, row block)
    void* const* grads;   // in: G_0, out: residual
    void* out;            // flat output (written when write_out)
    const float* x;       // in-factor, Q layout (orthonormal, or raw when ss_in is set)
    Terms res;            // local terms of the earlier iterations (also the output terms at W = 1)
    int32_t nres;
    int32_t write_out;    // world size 1: output = sum of all terms
    float* yloc;          // P local -> history
    float* state;         // P local -> reference-visible state buffer
    // rank-1 fused normalisation of the raw in-factor (as ReduceArgs): per row block its
    // group's range of `ss_in` is rng[block].g[rsel] (rsel 0: the even reduction's items, 1: the
    // items after an odd-even pass)
    const float* ss_in;
    const FinRng* rng;
    int32_t rsel;
    float* xstate;
    float* hx;
    int32_t ntiles;       // row blocks; flat pack items come first (as ApplyArgs)
    FlatArgs flat;
    // projection form (nres = kFinProj, see psgd_final.cuh): P_0 rows and R' per matrix
    const float* proj_p0;  // P layout
    const float* proj_r;   // Q layout: R' (r x r, row-major) at each matrix's qoff
    // (rank-1 projection form: ||Q_0,i||^2 of the matrix against the group norm sums the
    // matrix's even reduction items, rng[block].mb .. me of ss_in)
    float* xout;           // one-shot exchange: P local also to this rank's exchange slot, or null
    int32_t out_nt;        // output stores nt only (large plans), else write-through (psgd_stream.cuh)
    // odd-even pass (k_final_oe): no residual / output stores; per row block the next (even)
    // iteration's raw product sum_rows (g - P x^T) P and sum_rows P^2 (MatDesc::oe_part / oe_blk0)
    float* oe_part;
    float* oe_ss;
};
hipError_t launch_final_oe(int dtype, int nres, int smax, const FinalArgs& a, int ntiles, hipStream_t s, int* waves);
// nres value selecting the projection form of the fused final pass (I = 2, world size 1)
constexpr int kFinProj = 1000;
// rows per row block of the register-panel final pass (the projection form stages a block's
// P_0 rows in LDS)
constexpr int kFinRowsMax = 256;

struct OrthArgs {
    const OrthUnit* units;
    float* state;        // in-factor state buffer, orthonormalised in place
    float* hx;           // history copy of the orthonormal in-factor
    float* save;         // if non-null: copy of the pre-orthonormalisation values
    int32_t flags;       // diagnostics (PSGD_ORTH_DIAG): 1 = skip the Householder fallback
    // if non-null (Cholesky-QR kernels k_orth_chol<R>): the QR factor R' of each panel,
    // input panel = orthonormal output x R' (upper triangular r x r, row-major, written at the
    // unit's offset; rank-1 units: the joint-norm divisor at every panel's offset)
    float* rfac;
};

// ------------------------------------------------------------------ fp64 gradients
// The reference's own error-feedback test runs in float64 (tests/powersgd_test.py:38); its P/Q
// then follow the default dtype (powersgd.py:241-251), so gradients, factors and arithmetic are
// all fp64 (psgd_f64.hip). Same plan layout (MatDesc, OrthUnit, P/Q offsets) as fp32.
constexpr int kF64Cols = 64;    // even product: columns per tile (one per lane)
constexpr int kF64Rows = 256;   // even product: rows per chunk (partials per chunk)
constexpr int kF64OddRows = 16; // odd product: rows per workgroup (4 per wave)

struct TermsF64 {
    const double* p[kMaxTerms];
    const double* q[kMaxTerms];
};

struct F64Args {
    const MatDesc* mats;
    const Tile* tiles;
    void* const* grads;       // G_0 (in), residual (out, apply)
    const double* x;          // orthonormal in-factor (products)
    double* part;             // even partials [nchunk][m][r] per matrix at part_off[mat]
    const int64_t* part_off;
    double* y;                // out-factor state (reduce / odd product)
    double* yh;               // its history copy
    TermsF64 res;             // local terms (products: earlier iterations; apply: all)
    int32_t nres;
    TermsF64 apx;             // all-reduced terms (apply), scaled by alpha
    double alpha;
    void* out;                // flat output (apply)
    const RedItem* items;     // even reduction items
};

struct F64OrthArgs {
    const OrthUnit* units;
    double* state;            // in-factor, orthonormalised in place
    double* hx;               // history copy of the result
    double* save;             // if non-null: copy of the values before orthonormalisation
};

hipError_t launch_f64_product(bool even, int R, const F64Args& a, int ntiles, hipStream_t s);
hipError_t launch_f64_reduce(int R, const F64Args& a, int nitems, hipStream_t s);
hipError_t launch_f64_apply(int R, const F64Args& a, int ntiles, hipStream_t s);
hipError_t launch_f64_orth(int R, const F64OrthArgs& a, int nunits, hipStream_t s);

// ------------------------------------------------------------------ wide ranks (33-128)
// fp32/bf16 plans whose rank bucket is 64 or 128 (psgd_wide.hip): the products and the apply
// pass on v_mfma_f32_16x16x4_f32, their own tiles and partials, none of the fused forms. Same
// plan layout (MatDesc, OrthUnit, P/Q offsets, factor history) as the ranks <= 32. MatDesc
// fields as the wide tiling uses them (psgd_plan::set_wide_tiles):
//   even product: tile (mat, strip = 64-column block, chunk = block of chunk_rows rows),
//                 partials [nchunk][m][r] at part_even (floats from the wide partial region)
//   odd product:  tile (mat, strip = block of odd_sw columns, chunk = 64-row block),
//                 partials [odd_nstrip][n][r] at part_odd
//   apply:        tile (mat, strip = block of kWideApplyCols columns, chunk = 64-row block)
constexpr int kWideOut = 64;        // out-factor rows per workgroup (16 per wave)
constexpr int kWideStep = 64;       // summed gradient rows / columns per loop step
constexpr int kWideApplyCols = 256; // columns per apply tile

struct WideArgs {
    const MatDesc* mats;
    const Tile* tiles;
    void* const* grads;       // G_0 (in), residual (out, apply)
    const float* x;           // orthonormal in-factor (products)
    float* part;              // wide partial region
    Terms res;                // local terms (products: earlier iterations; apply: all)
    int32_t nres;
    Terms apx;                // all-reduced terms (apply), scaled by alpha
    float alpha;
    int32_t shared;           // apply: apx == res and alpha == 1 (world size 1)
    void* out;                // flat output (apply)
    float* y;                 // out-factor state (reduce)
    float* yh;                // its history copy
    const RedItem* items;     // reduction items (mat, start, cnt, np)
    int32_t even;
    float* xout;              // IPC exchange: the local out-factor also to this rank's slot, or null
};
hipError_t launch_wide_product(int dtype, int R, bool even, const WideArgs& a, int ntiles, hipStream_t s);
hipError_t launch_wide_reduce(const WideArgs& a, int nitems, hipStream_t s);
hipError_t launch_wide_apply(int dtype, int R, const WideArgs& a, int ntiles, hipStream_t s);
// Orthonormalisation of a wide plan's units in three launches (psgd_wide.hip): the panels' Gram
// matrices over row blocks of kWideGramRows rows, one workgroup per unit for the r x r chain
// (rank-1 units: the joint group norm; rejected panels: Householder QR), then Y = X M' over the
// same row blocks.
constexpr int kWideGramRows = 512;
struct WideOrthArgs {
    const OrthUnit* units;
    const Tile* items;     // (mat = unit, strip = row block of the panel, chunk = partial slot)
    const int32_t* slot0;  // per unit: its first partial slot
    float* state;          // in-factor state buffer, orthonormalised in place
    float* hx;             // history copy of the orthonormal in-factor
    float* save;           // if non-null: copy of the pre-orthonormalisation values
    double* gram;          // per slot an R x R Gram partial (blocks on and above the diagonal)
    double* m;             // per unit M = R^-1 (R x R, row-major, upper triangular)
    double* sg;            // per unit LAPACK's column signs (R entries)
    int32_t* ok;           // per unit: 1 = the panel is X M D (third launch), 0 = already done
};
hipError_t launch_wide_orth(int R, const WideOrthArgs& a, int nunits, int nitems, hipStream_t s);

// Host-side launchers, grouped by the unit that defines them. Return hipError_t.
// psgd_step.cpp: by dtype to the launchers of psgd_{product,apply,final}_{f32,bf16}.hip and
// psgd_f64.hip (psgd_plan.h)
hipError_t launch_odd_mfma(int dtype, int R, int nres, const ProductArgs& a, int ntiles,
                           hipStream_t s);
hipError_t launch_apply(int dtype, int R, int nterms, bool shared, const ApplyArgs& a,
                        int ntiles, hipStream_t s);
// ntiles == 0: no launch, only the occupancy query (*waves = resident waves per SIMD)
hipError_t launch_final_odd(int dtype, int R, int nres, int smax, const FinalArgs& a, int ntiles,
                            hipStream_t s, int* waves = nullptr);
hipError_t launch_lowrank_out(int dtype, int R, int nterms, const ApplyArgs& a, int ntiles, hipStream_t s);
// psgd_reduce.hip
hipError_t launch_reduce(const ReduceArgs& a, int nitems, hipStream_t s);
// psgd_orth.hip
hipError_t launch_orth(const OrthArgs& a, int nunits, int R, int64_t max_rows, bool chol, hipStream_t s);
hipError_t launch_orth_chain(const ChainArgs& a, int nunits, int64_t max_rows, int R, hipStream_t s);
// paper-code Gram-Schmidt (gradient_reducers.py:945-956) on one panel per unit, per matrix
hipError_t launch_orth_mgs(const OrthArgs& a, int nunits, int R, hipStream_t s);
// psgd_pack.hip (fp64: psgd_f64.hip)
hipError_t launch_flat_pack(int dtype, const FlatArgs& a, hipStream_t s);
hipError_t launch_flat_pack_f64(const FlatArgs& a, hipStream_t s);

// DDP bucket <-> parameter tensors (psgd_runs_*): one work item = up to kRunItem consecutive
// elements of one run; k_runs<ADD> adds the bucket into the tensors or gathers them into it.
constexpr int kRunItem = 16 * kBlock;
struct RunItem {
    int64_t boff, toff;  // element offsets in the bucket / in the tensor
    int32_t tensor, cnt; // tensor index, elements (<= kRunItem)
};
struct RunsArgs {
    const RunItem* items;
    void* bucket;
    void* const* tensors;
    int32_t nitems;
};
hipError_t launch_runs(int dtype, bool add, const RunsArgs& a, hipStream_t s);  // psgd_pack.hip

// The run tables of psgd_runs_create_mixed that k_runs does not serve: a bf16 bucket side over
// fp32 tensors (the fp32 error-feedback residual of bf16 gradients), and the source-table form,
// where item i's bucket side is sources[src[i]] instead of one base pointer (`src` null: `bucket`).
enum RunsMode { kRunsGather = 0, kRunsAdd = 1, kRunsAddZero = 2 };  // AddZero: ADD, then bucket = +0.0
struct RunsMixArgs {
    const RunItem* items;
    const int32_t* src;      // per item: its source index (source-table form), else null
    void* bucket;            // single-bucket form
    void* const* sources;    // source-table form
    void* const* tensors;
    int32_t nitems;
};
hipError_t launch_runs_mix(int bucket_dtype, int tensor_dtype, int mode, const RunsMixArgs& a, hipStream_t s);

// psgd_aggregate_mixed (fp32 plans at world size 1, rank buckets 1 / 2 / 4 / 16 / 32): the fp32
// codec on an fp32 error-feedback residual fed by bf16 gradients, with the two element-wise passes
// around it folded into its own gradient passes. The mixed kernel instances take this second argument
// beside the codec's own (whose structs, and so every other instance, stay as they are):
//   output fold   the step's final pass (k_final_odd / k_final_proj / k_apply) stores its output
//                 as bf16 (StIo<bf16_t>; `out` and the flat buffer are bf16 buffers); the residual
//                 stays fp32
//   ingest fold   the single-pass k_final_odd (I = 1, odd step: the step's only gradient pass)
//                 loads residual + float(src) (ONE fp32 add) and stores +0.0 to src beside its own
//                 residual. (The same fold in k_even was built and measured slower than the
//                 run-table ADD it replaces, DESIGN.md section 10: not kept.)
//   flat items    an uncompressed tensor's item does both: flat = bf16(x + float(src)), x = src = +0.0
// psgd_aggregate_mixed_comm (world size W over a communicator) keeps the output fold only: the
// final pass of the W > 1 sequence (k_apply with two term sets, or k_lowrank_out after a fused
// k_final_odd) stores bf16. The all-reduce sums fp32 values, so the uncompressed tensors travel
// through `stage` (fp32, the flat plan's layout, owned by the plan):
//   ingest-pack   stage = (x + float(src)) / W, x = src = +0.0   a launch of its own, before the
//                 first collective (flat_ingest_item)
//   round         flat = bf16(stage)   leading workgroups of the final launch (flat_round_item)
struct MixArgs {
    void* const* src;      // bf16 gradients of the plan's tensors (gradient-table order), ingest fold
    void* const* unc_src;  // bf16 gradients of the uncompressed tensors (the flat plan's order)
    float* stage;          // psgd_aggregate_mixed_comm: fp32 staging of the flat tail, else null
};
// psgd_mixed_{final,apply}.hip. ntiles == 0: no launch; `*waves` (if non-null) receives
// the resident waves per SIMD of the instance that would run, 0 when it uses scratch.
hipError_t launch_final_mix(int R, int nres, int smax, bool ingest, const FinalArgs& a, const MixArgs& x, int ntiles,
                            hipStream_t s, int* waves);
hipError_t launch_apply_mix(int R, int nterms, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s,
                            int* waves);
// psgd_mixed_comm.hip: the final pass of psgd_aggregate_mixed_comm at W > 1 (`waves` as above).
// launch_apply_mix_w: k_apply's two-term-set form with the output stored as bf16;
// launch_lowrank_mix: k_lowrank_out's (the output pass after a fused k_final_odd), rank buckets 1 / 2.
// In both, a.flat's items are round items (flat_round_item) and come first. launch_flat_ingest /
// launch_flat_round: the flat items as launches of their own.
hipError_t launch_apply_mix_w(int R, int nterms, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s,
                              int* waves);
hipError_t launch_lowrank_mix(int R, int nterms, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s,
                              int* waves);
hipError_t launch_flat_ingest(const FlatArgs& a, const MixArgs& x, hipStream_t s);
hipError_t launch_flat_round(const FlatArgs& a, const MixArgs& x, hipStream_t s);

// psgd_aggregate_mixed_comm_dst (the DDP hook's one-call form): the final pass of the
// communicator sequence stores each tensor's bf16 average at the tensor's own destination (a view
// into a DDP bucket: dense, 2-byte aligned or better) instead of a dense buffer at the plan's
// output offsets. Device pointer tables: `dst` in the plan's tensor order (the launch functions
// read it as ApplyArgs::odst), `unc_dst` in the flat plan's order (a kernel argument of its own
// beside MixArgs, whose layout the existing instances keep). The tiles are laid out exactly as
// the dense instances' (from the residual's alignment); only their stores follow the
// destination's alignment (psgd_stream.cuh, apply_tile).
struct MixDst {
    void* const* dst;
    void* const* unc_dst;
};
// psgd_mixed_dst.hip: the destination-table instances of launch_apply_mix_w, launch_lowrank_mix
// and launch_apply_mix (`waves` as above). The first two carry a.flat's items as round items into
// unc_dst, first; launch_apply_mix_dst (a 1-rank communicator's unfused final pass) takes none:
// launch_flat_round_dst follows it as a launch of its own.
hipError_t launch_apply_mix_w_dst(int R, int nterms, const ApplyArgs& a, const MixArgs& x, void* const* unc_dst,
                                  int ntiles, hipStream_t s, int* waves);
hipError_t launch_lowrank_mix_dst(int R, int nterms, const ApplyArgs& a, const MixArgs& x, void* const* unc_dst,
                                  int ntiles, hipStream_t s, int* waves);
hipError_t launch_apply_mix_dst(int R, int nterms, const ApplyArgs& a, int ntiles, hipStream_t s, int* waves);
hipError_t launch_flat_round_dst(const FlatArgs& a, const MixArgs& x, void* const* unc_dst, hipStream_t s);
// psgd_mixed_mfma.hip: rank buckets 16 / 32 of launch_apply_mix, launch_apply_mix_w,
// launch_apply_mix_w_dst and launch_apply_mix_dst (which hand them their cases 16 and 32): the
// matrix-core tile of k_apply<float> with the output stored as bf16, its VALU fallback where
// k_apply takes it. One instance per (R, term sets, ONT / destination form): no terms are cached
// at these ranks. Any other R: hipErrorInvalidValue (rank bucket 8 has no mixed instance).
hipError_t launch_apply_mix_mc(int R, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s, int* waves);
hipError_t launch_apply_mix_w_mc(int R, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s, int* waves);
hipError_t launch_apply_mix_w_dst_mc(int R, const ApplyArgs& a, const MixArgs& x, void* const* unc_dst, int ntiles,
                                     hipStream_t s, int* waves);
hipError_t launch_apply_mix_dst_mc(int R, const ApplyArgs& a, int ntiles, hipStream_t s, int* waves);

// psgd_aggregate_comm_dst / psgd_aggregate_ipc_dst (the default fp32 DDP hook's one-call form): the
// final pass of an fp32 plan (rank buckets 1-32) stores each tensor's fp32 average at the tensor's
// own destination (a view into a DDP bucket: dense, 4-byte aligned or better) instead of the
// output slab. `dst` in the plan's tensor order (read as ApplyArgs::odst), `unc_dst` in the flat
// plan's order; `stage` the plan-owned fp32 buffer the flat tail's collective (or last exchange)
// summed into, in the flat plan's layout. The tiles are laid out exactly as the dense instances'
// (from the gradients' alignment and the plan's offsets); only their output stores follow the
// destination's alignment.
struct DirectDst {
    void* const* dst;
    void* const* unc_dst;
    float* stage;
};
// psgd_apply_dst.hip: the destination-table instances of k_apply<float> (shared: the 1-rank
// communicator's; else two term sets) and of k_lowrank_out<float> (rank buckets 1 / 2). a.flat's
// items are copy items (unc_dst[k] = stage) and come first. ntiles + items == 0: no launch;
// `*waves` (if non-null) receives the resident waves per SIMD of the instance that would run, 0
// when it uses scratch.
hipError_t launch_apply_dst(int R, int nterms, bool shared, const ApplyArgs& a, const DirectDst& t, int ntiles,
                            hipStream_t s, int* waves);
hipError_t launch_lowrank_dst(int R, int nterms, const ApplyArgs& a, const DirectDst& t, int ntiles, hipStream_t s,
                              int* waves);

// One-shot all-reduce over IPC-mapped exchange buffers (psgd_aggregate_ipc). Every rank's
// exchange buffer: kXchgHeader bytes of per-iteration epoch flags (uint64, one per iteration),
// then two parities x iterations slots of xchg_slot floats each; the producer kernels (k_reduce,
// k_final_odd, the flat pack) write the LOCAL factor into this rank's slot, and k_xchg raises
// this rank's flag, waits (bounded) for every peer's flag and sums the W slots in rank order.
constexpr int kMaxRanks = 64;
constexpr int64_t kXchgHeader = 256;
// byte offset, in the header, of the device copy of the sticky error word (XchgArgs::err_dev):
// past the flags of every iteration (num_iters_per_step <= kMaxTerms)
constexpr int64_t kXchgErrOff = 192;
// byte offset of this buffer's session nonce (uint32, written at psgd_ipc_create): peers check it
// through their mapping at psgd_ipc_open, and every epoch flag carries it in its high word, so a
// mapping that does not reach THIS session's buffer (a runtime that hands back a stale mapping
// of a freed buffer with an identical handle) fails loudly instead of summing stale slots
constexpr int64_t kXchgNonceOff = 200;
static_assert(kMaxTerms * 8 <= kXchgErrOff && kXchgErrOff + 4 <= kXchgNonceOff && kXchgNonceOff + 4 <= kXchgHeader,
              "exchange header layout");
struct XchgArgs {
    const char* const* peers;  // device array: the W exchange buffers (rank order, own included)
    uint64_t* own_flag;        // this rank's flag of this iteration (its own buffer)
    int64_t flag_off;          // byte offset of this iteration's flag in every buffer
    int64_t slot_off;          // byte offset of this step/iteration's slot in every buffer
    float* dst;                // SUM of the factors (the reference-visible state) ...
    int64_t n;                 // ... n floats
    float* flat_dst;           // SUM of the packed uncompressed tensors (last iteration) ...
    int64_t flat_off;          // ... at slot + flat_off floats
    int64_t nflat;
    uint64_t epoch;            // step + 1 (< 2^32)
    const uint32_t* nonces;    // device array: every rank's session nonce (flag = nonce << 32 | epoch)
    uint32_t own_nonce;
    uint32_t spin_limit;       // polls (~0.25 us apart) before a wait gives up
    int32_t world, rank;
    int32_t* err;              // set to 1 when a wait timed out (psgd_ipc_status; host-mapped)
    int32_t* err_dev;          // device copy of `err` (this rank's buffer header, kXchgErrOff):
                               // once set, later exchanges skip their waits and write NaN sums
    // rank-1 norm fold (non-last iterations): one workgroup per reduction item of this parity
    // (items, nitems, mats, even) writes the sum to dst and dst2 (the raw copy the next
    // iteration's kernels normalise on the fly) and the item's sum of squares to ss_out
    const RedItem* items;
    const MatDesc* mats;
    float* dst2;
    float* ss_out;
    int32_t nitems, even;
    // ranks 2/4, two iterations: the upper Gram of each item's rows of the SUMMED Q (fp64,
    // kGramStride per item) for k_orth_chain, as k_reduce leaves it at world size 1
    double* gram;
    int32_t gram_r;
};
hipError_t launch_xchg(const XchgArgs& a, hipStream_t s);  // psgd_xchg.hip

// Two-shot all-reduce of one factor over the same slots, flags and arguments (psgd_xchg2.hip;
// sessions of psgd_ipc_create2 on a wide plan): k_xchg_rs sums this rank's shard of the W slots
// into `dst` and, in place, into its own slot (epoch 2 * (step + 1) - 1); k_xchg_ag, the next
// launch, copies every other rank's shard from that rank's slot and, on the last iteration, sums
// the flat tail one-shot (epoch 2 * (step + 1)). launch_xchg_rs ignores the flat fields.
// The partition (psgd_ipc_shard): contiguous shards of xchg_shard_quads(n, W) 16-byte quads, the
// last non-empty one clipped to n, later ones empty.
__host__ __device__ inline int64_t xchg_shard_quads(int64_t n, int32_t world) {
    return ((n + 3) / 4 + world - 1) / world;
}
hipError_t launch_xchg_rs(const XchgArgs& a, hipStream_t s);
hipError_t launch_xchg_ag(const XchgArgs& a, hipStream_t s);
// psgd_ipc_create2, mode auto: an exchange runs two-shot when the session's world is >= 3 (at
// W = 2 the remote bytes are equal and only the extra launch remains) and the factor is at least
// this many bytes. DESIGN section 11's estimate ("factors above ~0.5 MB"): nobody has measured it,
// and it cannot be measured on one GPU.
constexpr int64_t kXchgTwoShotBytes = int64_t(512) << 10;

// The LAST exchange of psgd_aggregate_mixed_ipc[_dst] when the step has a flat tail (k_xchg_mix,
// psgd_xchg_mix.hip): the factor exactly as k_xchg (never the item / Gram form: those belong to
// non-last iterations), the flat region of the slot (XchgArgs::flat_off, the flat plan's layout)
// summed per flat item and stored as bf16 where the averages belong: the dense bf16 flat buffer
// at the flat plan's offsets (`flat_out`), or each tensor's own destination (`unc_dst`, the flat
// plan's order: the destination-table form). No fp32 copy of the flat sums exists (XchgArgs::
// flat_dst unused).
struct XchgMixArgs {
    const FlatEntry* entries;
    const FlatItem* items;
    int32_t nitems;
    void* flat_out;          // bf16, dense form
    void* const* unc_dst;    // bf16 destinations, destination-table form
};
hipError_t launch_xchg_mix(const XchgArgs& a, const XchgMixArgs& m, bool dst, hipStream_t s);

}  // namespace psgd
