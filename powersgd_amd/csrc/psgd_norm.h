// Global-norm clipping of a step's averages (psgd_clip_outputs, include/psgd.h): the argument
// structs and launchers shared by the driver (psgd_norm.cpp) and the kernels (psgd_norm.hip).
//
// A compressed tensor's average is A = alpha * sum_k P_k Q_k^T over the term set the output pass
// read (ApplyArgs::apx). With the terms stacked, P^ = [P_0 .. P_{I-1}] (n x K, K = I * r) and Q^
// likewise,  ||A||_F^2 = alpha^2 <P^^T P^, Q^^T Q^>_F : two K x K Gram matrices per matrix, from
// the factors alone (factor form). The cross blocks between iterations stay in: they vanish only
// where every in-factor is orthonormal per matrix, which a jointly normalised rank-1 shape group
// is not. Everything that has no factors (uncompressed tensors, warm-up steps, wide / fp64 plans)
// is a fixed-order sum of squares over a dense range (stream form).
#pragma once

#include "psgd_internal.h"

namespace psgd {

constexpr int kNormMaxK = 64;      // stacked width I * rank bucket the factor form serves
constexpr int kNormChunk = 32;     // factor rows staged in LDS per pass of k_norm_gram at the widest stack
constexpr int kNormVecs = 4096;    // 16-byte vectors per workgroup of k_norm_scale
constexpr int kNormStreamWg = 2048;  // at most this many workgroups (partials) per range of k_norm_stream

// k_norm_gram work item: rows [row0, row0 + rows) of one side's stacked factor of one matrix;
// its partial (the upper triangle of the Gram, K (K + 1) / 2 doubles, row-major) at `part`
struct NormItem {
    int32_t mat, side;  // side 0: P (n rows), 1: Q (m rows)
    int32_t row0, rows;
    int64_t part;       // doubles from the partial buffer
};
// per matrix (plan order): its items of both sides, each side's contiguous and in row order
struct NormMat {
    int32_t item0[2], nitems[2];
};

struct NormGramArgs {
    const MatDesc* mats;
    const NormItem* items;
    Terms apx;        // the step's output terms (fp32 factors)
    int32_t nterms;
    double* part;
};
struct NormMatArgs {
    const MatDesc* mats;
    const NormItem* items;
    const NormMat* nmats;
    const double* part;
    int32_t nterms;
    double alpha;     // 1 / world, as the output pass rounded it to fp32
    double* sq;       // per tensor (MatDesc::tensor): alpha^2 <G_P, G_Q>
};
// two dense ranges: workgroups [0, nwg[0]) serve range 0, the next nwg[1] range 1
struct NormRangeArgs {
    void* base[2];
    int64_t numel[2];
    int32_t nwg[2];
};
// psgd_clip_dst: the scale pass through per-tensor destination tables (table 0: the plan's tensors,
// table 1: the flat plan's). One work item = up to kNormDstItem consecutive elements of one
// destination, starting at a multiple of kNormDstItem: the item's pointer has its destination's
// alignment modulo 16 bytes. Built on the host from the numels alone.
constexpr int kNormDstVecs = 8;                          // 16-byte vectors per thread of an item
constexpr int kNormDstItem = kNormDstVecs * kBlock * 4;  // fp32 elements: half of k_norm_scale's workgroup
static_assert(kNormDstItem % 4 == 0 && kNormDstItem <= kNormVecs * 4, "item length");
struct NormDstItem {
    int64_t off;          // elements from the destination's first
    int32_t tensor, cnt;  // index into the item's table; elements (<= kNormDstItem)
};
// workgroups [0, nitems[0]) serve table 0's items, the next nitems[1] table 1's
struct NormDstArgs {
    const NormDstItem* items[2];
    void* const* table[2];
    int32_t nitems[2];
};
struct NormFinishArgs {
    const double* sq;     // factor form: per-tensor squares, nsq of them (tensor order); else null
    int32_t nsq;
    const double* part;   // k_norm_stream partials: range 0's npart[0], then range 1's npart[1]
    int32_t npart[2];
    double max_norm;
    double* result;       // norm, coef
};

// psgd_norm.hip. `ept`: upper-triangle entries per thread of the instance (1, 2, 4 or 9: stacked
// widths up to 22 / 31 / 44 / 64). The stream-form workgroups of the dense ranges `rg` (the
// uncompressed slab; partials to `spart` as launch_norm_stream leaves them) ride in the same launch.
hipError_t launch_norm_gram(int ept, const NormGramArgs& a, int nitems, int dtype, const NormRangeArgs& rg,
                            double* spart, hipStream_t s);
hipError_t launch_norm_mat(const NormMatArgs& a, int nmats, hipStream_t s);
hipError_t launch_norm_stream(int dtype, const NormRangeArgs& r, double* part, hipStream_t s);
hipError_t launch_norm_finish(const NormFinishArgs& a, hipStream_t s);
hipError_t launch_norm_scale(int dtype, const NormRangeArgs& r, const double* result, hipStream_t s);
hipError_t launch_norm_scale_dst(const NormDstArgs& a, const double* result, hipStream_t s);  // fp32
// resident waves per SIMD of every instance (0: scratch), for the admission check and tools
int norm_min_waves();

}  // namespace psgd
