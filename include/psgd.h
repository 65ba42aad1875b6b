/*
 * psgd.h — C ABI of the MI355X-native PowerSGD codec (libpsgd.so).
 *
 * Drop-in boundary for the hot path of epfml/powersgd. Every entry point names the
 * reference interface it replaces (paths relative to the reference repository):
 *
 *   psgd_should_compress   powersgd/powersgd.py:101-105 (+ avg_compressed_size :292-294)
 *   psgd_plan_create       BasicPowerSGD.__init__       powersgd/powersgd.py:114-144, :253-263
 *   psgd_plan_* queries    _ps_buffer/_qs_buffer layout :130-144, compression_rate :265-275
 *   psgd_compress          one power iteration          powersgd/powersgd.py:172-202
 *                          (orthogonalize :188 -> orthogonalization.py:4-8; bmm :189-193;
 *                           local error-feedback update :195-202)
 *   psgd_decompress        approximation + un-batching  powersgd/powersgd.py:211-230
 *   psgd_plan_fused_final  (which final-pass form a step takes; no reference counterpart)
 *   psgd_*_bucket          the same per bucket of shape groups, for comm/compute overlap of the
 *                          factor all-reduce (powersgd.py:204-209 split into slices)
 *   psgd_aggregate         BasicPowerSGD.aggregate      powersgd/powersgd.py:146-235 (world size 1)
 *   psgd_flat_*            AllReduce.aggregate          powersgd/powersgd.py:22-31,
 *                          pack / allreduce_average      powersgd/utils.py:6-10, :43-49
 *   psgd_aggregate_flat    PowerSGD.aggregate           powersgd/powersgd.py:64-74 (world size 1)
 *   psgd_aggregate_comm    PowerSGD.aggregate at world size W over RCCL (:64-74, :204-209)
 *   psgd_aggregate_ipc     the same over IPC exchange buffers with device-side flags (one node)
 *   psgd_aggregate_mixed   the world-size-1 step on an fp32 residual fed by bf16 gradients, the
 *                          element-wise passes around the codec folded into it
 *   psgd_runs_*            DDP comm-hook plumbing: a DDP bucket's flat buffer
 *                          <-> the per-parameter tensors, by a run table; the error-feedback add
 *                          the reference gets from autograd's accumulation into p.grad
 *                          (README.md:39-42, powersgd/__init__.py:24-25) and the per-bucket
 *                          gather of the averaged gradients (paper-code/train_pytorch.py:106-131)
 *   psgd_clip_outputs      torch.nn.utils.clip_grad_norm_ on what a step returned, from the
 *                          low-rank factors where the plan has them (no reference counterpart)
 *   psgd_clip_dst          the same after a direct-store completion: the averages scaled where
 *                          they lie, inside the DDP buckets
 *   psgd_guard_outputs     skip a step whose aggregates are not finite, decided and carried out
 *                          on the device: zero averages and residual, P / Q back to their seed
 *
 * Conventions
 *  - No torch types. Device buffers are plain pointers on the plan's device; `stream` is a
 *    hipStream_t passed as void*. All compute calls are stream-ordered and asynchronous, do no
 *    device allocation and no host synchronisation (except a one-off pointer-table upload when
 *    the set of gradient pointers changes).
 *  - Ownership: the caller owns gradients, outputs, the P/Q state buffers and the workspace;
 *    the plan owns host-side layout only.
 *  - Gradients are mutated in place into the error-feedback residual (reference :230).
 *  - P/Q factors are fp32 for fp32/bf16 gradients and fp64 for fp64 gradients (reference
 *    :241-251 allocates them in the default dtype, which must match the gradients' for its bmm).
 *  - The building blocks (psgd_product / psgd_orthogonalize / psgd_reconstruct) and the fused
 *    fp32 kernels take fp32/bf16 plans only (PSGD_ERR_DTYPE for an F64 plan).
 *  - Rank limit: the effective rank min(rank, n, m) of every matrix is at most 128 for
 *    fp32/bf16 plans and at most 32 for fp64 plans (PSGD_ERR_VALUE at psgd_plan_create). A plan
 *    whose largest effective rank exceeds 32 is a WIDE plan (psgd_plan_is_wide): same P/Q layout,
 *    its own matrix-core kernels, none of the fused forms. psgd_compress, psgd_decompress,
 *    psgd_aggregate, psgd_aggregate_flat, psgd_aggregate_comm, psgd_aggregate_ipc (over a session
 *    of psgd_ipc_create2), the timing calls and every psgd_plan_* query take wide plans;
 *    psgd_plan_set_buckets with more than one bucket, the *_bucket calls, the building blocks and
 *    psgd_ipc_create refuse them (PSGD_ERR_VALUE, nothing is launched).
 *  - Errors: every call returns a psgd_status; psgd_last_error() returns a thread-local message.
 *    PSGD_ERR_INDEX mirrors the reference's IndexError (no tensors, :118), PSGD_ERR_DTYPE its
 *    RuntimeError on unsupported dtypes (:189), PSGD_ERR_LAYOUT its RuntimeError on
 *    non-viewable tensors (:289).
 *  - Not re-entrant per plan; one plan per device/process (reference: single-threaded, :146).
 *  - Stream order: the calls of one plan must be ordered on ONE stream (as torch's current
 *    stream orders them). The plan's device pointer tables are re-uploaded on the launch stream
 *    when the gradient pointer set changes; a kernel of an earlier call still running on another
 *    stream could read a slot being rewritten.
 */
#ifndef PSGD_H
#define PSGD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psgd_plan psgd_plan;
typedef struct psgd_flat psgd_flat;
typedef struct psgd_comm psgd_comm;
typedef struct psgd_runs psgd_runs;

enum psgd_status {
    PSGD_OK = 0,
    PSGD_ERR_INDEX = 1,   /* empty tensor list (reference IndexError)              */
    PSGD_ERR_VALUE = 2,   /* invalid argument (rank < 1, iterations out of range…) */
    PSGD_ERR_DTYPE = 3,   /* unsupported dtype                                      */
    PSGD_ERR_LAYOUT = 4,  /* unsupported layout / empty tensor                      */
    PSGD_ERR_DEVICE = 5,  /* HIP runtime error                                      */
    PSGD_ERR_STATE = 6    /* call order error (e.g. compute before psgd_plan_bind)  */
};

/* Gradient dtypes. F32 / BF16: factors (P/Q state) and arithmetic fp32. F64: the reference's
 * own test dtype (tests/powersgd_test.py:38): factors and arithmetic fp64, as the reference's
 * default-dtype P/Q (powersgd.py:241-251) are then. */
enum psgd_dtype { PSGD_F32 = 0, PSGD_BF16 = 1, PSGD_F64 = 2 };

/* Largest num_iters_per_step a plan accepts. */
#define PSGD_MAX_ITERS 16

int psgd_version(void);
const char* psgd_last_error(void);

/* Compression policy: numel / (0.5*iters*min(rank,min(shape))*sum(shape)) > min_rate,
 * evaluated on the ORIGINAL tensor shape (reference powersgd.py:101-105, :292-294). */
int psgd_should_compress(const int64_t* shape, int32_t ndim, int32_t rank,
                         int32_t num_iters_per_step, double min_compression_rate,
                         int32_t* out_flag);

/* ---------------------------------------------------------------- codec plan ------ */
/* `dims` holds the concatenated shapes of the `num_tensors` compressed tensors
 * (ndims[i] entries each). Matrices are the view [shape[0], numel/shape[0]]; they are
 * grouped by matrix shape in first-appearance order, and the P (resp. Q) state buffer
 * is the concatenation over groups of [count, n, r] (resp. [count, m, r]) fp32 arrays,
 * r = min(rank, n, m) — byte-for-byte the reference's _ps_buffer/_qs_buffer layout.
 * The largest r may be 128 (fp32 / bf16) or 32 (fp64); beyond that PSGD_ERR_VALUE. */
int psgd_plan_create(const int64_t* dims, const int32_t* ndims, int32_t num_tensors,
                     int32_t rank, int32_t num_iters_per_step, int32_t dtype,
                     psgd_plan** out_plan);
int psgd_plan_destroy(psgd_plan* plan);

int psgd_plan_num_groups(const psgd_plan* plan, int32_t* out);
int psgd_plan_group(const psgd_plan* plan, int32_t g, int64_t* n, int64_t* m, int32_t* r,
                    int32_t* count);
int psgd_plan_factor_numel(const psgd_plan* plan, int64_t* p_numel, int64_t* q_numel);
/* Element offset of compressed tensor i inside the flat output buffer, and the total
 * number of elements that buffer needs. The layout is dense in tensor order (torch.cat). */
int psgd_plan_output_offset(const psgd_plan* plan, int32_t i, int64_t* offset);
int psgd_plan_output_numel(const psgd_plan* plan, int64_t* numel);
int psgd_plan_workspace_bytes(const psgd_plan* plan, int64_t* bytes);
/* reference compression_rate / uncompressed_num_floats / compressed_num_floats (:265-275) */
int psgd_plan_compression_rate(const psgd_plan* plan, double* rate, double* uncompressed,
                               double* compressed);

/* Bind caller-owned device memory: P state [p_numel] and Q state [q_numel] (fp32, or fp64
 * for a PSGD_F64 plan) and a workspace of psgd_plan_workspace_bytes() bytes (16-byte
 * aligned). Uploads the static layout tables (synchronous; call once). */
int psgd_plan_bind(psgd_plan* plan, int32_t device, void* p_state, void* q_state,
                   void* workspace);

/* Which state buffer iteration `it` of step `step` produces (and the caller must SUM-
 * all-reduce before the next call when world size > 1): 0 = Q (even), 1 = P (odd).
 * Parity = (step*num_iters_per_step + it) % 2 (reference :174). */
int psgd_out_factor(const psgd_plan* plan, int64_t step, int32_t it, int32_t* which);

/* One power iteration on every compressed matrix: orthonormalise the in-factor (rank 1:
 * one joint norm per shape group; rank > 1: Householder QR per matrix), then the
 * tall-skinny product with the error-feedback matrix G_it = G_0 - sum_{j<it} P_j Q_j^T
 * (formed on the fly). Leaves the LOCAL factor in the out-factor state buffer.
 * `grads[i]` = device pointer of compressed tensor i (contiguous).
 * Gradients are not written, EXCEPT by the last iteration of a step for which
 * psgd_plan_fused_final() reports 1: that iteration (odd, P = G X) is fused with the
 * final pass and leaves the error-feedback residual in `grads` (reference :195-202, :230);
 * psgd_decompress then only writes the output. */
int psgd_compress(psgd_plan* plan, void* const* grads, int64_t step, int32_t it, void* stream);

/* Fused final pass: grads[i] <- G_0 - sum_k P_k Q_k^T (local factors) and
 * out[i] <- (1/world_size) * sum_k P_k Qbar_k^T (all-reduced factors); `out` is the flat
 * output buffer (psgd_plan_output_offset). Call after the last psgd_compress (and its
 * all-reduce). */
int psgd_decompress(psgd_plan* plan, void* const* grads, void* out, int64_t step,
                    int32_t world_size, void* stream);

/* ------------------------------------------- buckets: comm/compute overlap (W > 1) ------ */
/* The reference all-reduces the whole out-factor buffer once per iteration (powersgd.py:
 * 204-209). With buckets, the shape groups are cut into `nbuckets` consecutive ranges
 * (group_end[b] = exclusive end group; the last must be psgd_plan_num_groups) and every launch of
 * an iteration can be issued per bucket: the caller all-reduces bucket b's slice of the factor
 * buffer (psgd_plan_bucket_range: element offset/length in the P and Q state buffers) as soon
 * as bucket b's kernels are queued, so that collective overlaps the next buckets' kernels. The
 * element-wise SUM over the slices equals the whole-buffer SUM. nbuckets = 0: one bucket (the
 * whole plan); at most 8 buckets. Synchronous (rewrites the tile tables): call between steps.
 * fp32/bf16 plans. */
int psgd_plan_set_buckets(psgd_plan* plan, int32_t nbuckets, const int32_t* group_end);
int psgd_plan_bucket_range(const psgd_plan* plan, int32_t bucket, int64_t* p_off, int64_t* p_len,
                           int64_t* q_off, int64_t* q_len);
/* psgd_compress / psgd_decompress restricted to one bucket's matrices (same semantics). */
int psgd_compress_bucket(psgd_plan* plan, void* const* grads, int64_t step, int32_t it, int32_t bucket,
                         void* stream);
int psgd_decompress_bucket(psgd_plan* plan, void* const* grads, void* out, int64_t step,
                           int32_t world_size, int32_t bucket, void* stream);

/* ------------------------- one-shot all-reduce over IPC, stream-ordered (W > 1, one node) ------ */
/* PowerSGD.aggregate at world size W (reference powersgd.py:64-74 with is_distributed(); the
 * factor all-reduce :204-209 and the uncompressed tensors' allreduce_average, utils.py:43-49)
 * without a collective library: one process per GPU, every rank reads all ranks' local factors
 * directly through IPC mappings (xGMI between GPUs) and sums them in rank order, so every rank
 * holds bitwise the same sum. Synchronisation is device-side: per iteration a kernel raises this
 * rank's epoch flag in its exchange buffer and polls the peers' flags (system scope, bounded: a
 * peer that never arrives sets the status word read by psgd_ipc_status instead of hanging).
 * No host barrier and no host synchronisation per step.
 * Exchange buffers are regions of a per-process, per-device arena that is allocated once and
 * never freed; every peer arena chunk is mapped once per process and never unmapped. A later
 * session of the same size gets the same region back: no free / malloc / re-map cycle between
 * sessions (a remapped, freed allocation can never alias a new session's buffer).
 *   psgd_ipc_create   takes this rank's exchange region (flags + two parities x iterations
 *                     slots, room for flat_numel uncompressed values), zeroes it, draws a fresh
 *                     session nonce into its header and exports arena handle + region offset +
 *                     nonce (psgd_ipc_handle_bytes bytes, the nonce last). Synchronous. Allowed
 *                     again after psgd_ipc_close (a new session on the same plan).
 *   psgd_ipc_open     the caller all-gathers the W handles (e.g. torch.distributed) and passes
 *                     them in rank order; maps each peer's arena chunk (first session only) and
 *                     reads each peer's nonce through the mapping: a mapping that does not reach
 *                     that session's region is PSGD_ERR_STATE, a list whose own entry is not this
 *                     rank's handle PSGD_ERR_VALUE. Every epoch flag carries its writer's nonce
 *                     in the high 32 bits and pollers accept only the nonce they opened with.
 *   psgd_aggregate_ipc the whole step on `stream` (same arguments as psgd_aggregate_comm).
 *   psgd_ipc_status   synchronous: 1 if a wait timed out since the last call (results invalid).
 *   psgd_ipc_close    synchronous: ends the session (mappings stay with the process). Teardown
 *                     is collective: every rank calls it, then the caller runs a cross-rank
 *                     barrier before any rank starts a new session or destroys the plan (its
 *                     region returns to the arena and a later session re-zeroes it).
 *   psgd_ipc_debug    diagnostics (tests): this process's arena counters, this session's region
 *                     address and nonce, and for peer w (open sessions) the mapped address and
 *                     the nonce read through the mapping. */
int psgd_ipc_handle_bytes(int64_t* bytes);
int psgd_ipc_create(psgd_plan* plan, int64_t flat_numel, void* handle_out);
int psgd_ipc_open(psgd_plan* plan, int32_t world_size, int32_t rank, const void* handles);
int psgd_aggregate_ipc(psgd_plan* plan, void* const* grads, void* out, int64_t step, psgd_flat* flat,
                       void* const* unc, void* flat_out, void* stream);
int psgd_ipc_status(psgd_plan* plan, int32_t* timed_out);
int psgd_ipc_close(psgd_plan* plan);
typedef struct psgd_ipc_info {
    int64_t arena_allocs;     /* arena chunks this process allocated (hipMalloc) */
    int64_t arena_opens;      /* peer chunks this process mapped (hipIpcOpenMemHandle) */
    int64_t arena_reuses;     /* regions served from chunks allocated earlier */
    int64_t arena_frees;      /* chunks freed: always 0 */
    uint64_t own_va;          /* this session's region */
    uint64_t peer_va;         /* peer w's region as mapped here (0 when no session is open) */
    uint32_t own_nonce;
    uint32_t peer_nonce_seen; /* the nonce in peer w's region header, read through the mapping */
} psgd_ipc_info;
int psgd_ipc_debug(psgd_plan* plan, int32_t peer, psgd_ipc_info* info);

/* The exchange for WIDE plans (effective ranks 33-128), and its two-shot form.
 * psgd_ipc_create keeps refusing a wide plan; psgd_ipc_create2 opens a session for either kind.
 * `mode`: 0 one-shot, 1 two-shot, 2 auto. Checked in this order: a null pointer or a mode outside
 * {0, 1, 2} PSGD_ERR_VALUE; an unbound plan PSGD_ERR_STATE; an fp64 plan PSGD_ERR_DTYPE; a plan
 * of rank <= 32 with mode 1 PSGD_ERR_VALUE (their non-last exchanges take per-item forms; two-shot
 * is not built for them); a negative flat_numel or a slot of 2^32 bytes or more PSGD_ERR_VALUE (the
 * kernels' buffer descriptors are 32-bit). On a plan of rank <= 32 with mode 0 or 2 it IS
 * psgd_ipc_create: the same region layout, flags, epochs, launches and results. On a wide plan it
 * opens a session that psgd_ipc_open, psgd_ipc_close, psgd_ipc_status, psgd_ipc_debug and
 * psgd_aggregate_ipc serve as above (psgd_aggregate_mixed_ipc[_dst] and psgd_aggregate_ipc_dst
 * keep refusing wide plans). Every rank of a session passes the same mode.
 *   One-shot: every rank reads all W slots whole, W * n floats per exchange of n floats, of which
 *   (W - 1) * n are remote.
 *   Two-shot: a reduce-scatter launch (rank r sums shard r of the W slots in rank order and
 *   stores the sum, in place, into its own slot) and an all-gather launch (every rank copies the
 *   other ranks' shards; on the last iteration it also sums the flat tail one-shot):
 *   2 * (W - 1) / W * n remote floats per rank, a factor W / 2 fewer (byte arithmetic). Every
 *   element is still summed in rank order, once, so the results are bitwise the one-shot ones
 *   on every rank. A timed-out wait leaves NaN in the shard (slot and state) and in every output.
 *   Auto: an exchange runs two-shot when the session's world is >= 3 and the factor is >= 512 KiB
 *   (an unmeasured estimate). A 1-rank session is always one-shot.
 * A wide plan's session uses two epochs per step on each iteration's flag word (2 * (step + 1) - 1
 * for the reduce-scatter phase, 2 * (step + 1) for the all-gather phase and for every one-shot
 * exchange), so psgd_aggregate_ipc then takes step < 2^31 - 1.
 *   psgd_ipc_two_shot  1 where the open session runs the factor exchange of `side` (0: P, the odd
 *                      iterations; 1: Q, the even ones) two-shot. PSGD_ERR_STATE without an open
 *                      session.
 *   psgd_ipc_shard     host only: the partition of n floats over `world_size` ranks the two-shot
 *                      kernels use. Contiguous shards in units of 4 floats,
 *                      ceil(ceil(n / 4) / world_size) quads each; the last non-empty shard is
 *                      clipped to n, later shards are empty (count 0). PSGD_ERR_VALUE for a null
 *                      pointer, n < 0, a world size outside 1..64 or a rank outside the world. */
int psgd_ipc_create2(psgd_plan* plan, int64_t flat_numel, int32_t mode, void* handle_out);
int psgd_ipc_two_shot(const psgd_plan* plan, int32_t side, int32_t* two_shot);
int psgd_ipc_shard(int64_t n, int32_t world_size, int32_t rank, int64_t* begin, int64_t* count);

/* Whole BasicPowerSGD.aggregate step for world size 1. */
int psgd_aggregate(psgd_plan* plan, void* const* grads, void* out, int64_t step, void* stream);

/* Nonzero when the last iteration of `step` is odd and every matrix fits the fused final
 * pass (row-resident product + residual, psgd_final.cuh). aggregate = 0: the building-block
 * path (psgd_compress of that iteration then writes the residual); aggregate = 1:
 * psgd_aggregate, which also fuses two-iteration rank-1/2/4 plans in the projection form
 * (output G X X^T, exact for I = 2 at world size 1): *fused = 2 for that
 * form (k_final_proj; ranks 1/2/4), 1 for the K-term form (k_final_odd), 0 unfused. */
int psgd_plan_fused_final(const psgd_plan* plan, int64_t step, int32_t aggregate, int32_t* fused);
/* Nonzero when iteration `it` of `step` (odd, followed by an even one) runs as ONE gradient pass
 * with the next iteration's product inside psgd_aggregate (rank 1, world size 1, I >= 3). */
int psgd_plan_odd_even(const psgd_plan* plan, int64_t step, int32_t it, int32_t* on);
/* 1 when the plan's largest effective rank exceeds 32 (rank bucket 64 or 128): the wide-rank
 * path. psgd_plan_fused_final and psgd_plan_odd_even report 0 for such a plan. */
int psgd_plan_is_wide(const psgd_plan* plan, int32_t* out);

/* Kernel timing for benchmarks: when enabled, every final pass launched by psgd_aggregate
 * (k_apply, or the fused final odd kernel) and by psgd_decompress (k_apply) is bracketed by HIP events recorded on its own stream.
 * psgd_plan_timing_read waits for the recorded events, returns the summed kernel time (ms)
 * and the number of launches, and clears the record. */
int psgd_plan_set_timing(psgd_plan* plan, int32_t enable);
int psgd_plan_timing_read(psgd_plan* plan, double* total_ms, int32_t* launches);

/* ------------------------------- building blocks (paper-code reducer variants) ------ */
/* The reference repository's paper code (paper-code/gradient_reducers.py) runs PowerSGD as
 * RankKReducer (:665-788) and HalfRankKReducer (:794-936) with a different call order. These
 * entry points expose the codec's kernels as steps so that such variants run on the same
 * plan, layout and kernels (powersgd_amd/reducers.py):
 *
 * psgd_product: y = G_k^T x (odd = 0; x P-layout, y Q-layout) or G_k x (odd = 1; x Q-layout,
 *   y P-layout) for every compressed matrix, G_k = G_0 - sum_{j<nterms} term_p[j] term_q[j]^T
 *   formed on the fly; no orthonormalisation (torch.matmul(matrix, q) :750 / matrix.t() @ p
 *   :770). y must not alias x or a term. */
int psgd_product(psgd_plan* plan, void* const* grads, int32_t odd, const float* x, float* y,
                 int32_t nterms, const float* const* term_p, const float* const* term_q, void* stream);
/* In-place orthonormalisation of every panel of a P-layout (which = 1) or Q-layout (0)
 * buffer. mode 0: the reference codec's (orthogonalization.py:4-8: joint rank-1 norm per
 * shape group, Householder QR above); mode 1: the paper code's Gram-Schmidt per matrix,
 * col /= sqrt(sum col^2) + 1e-8 (gradient_reducers.py:945-956). */
int psgd_orthogonalize(psgd_plan* plan, int32_t which, float* buf, int32_t mode, void* stream);
/* resid_out[i] <- G_0 - sum_k term_p[k] term_q[k]^T (null resid_out: back into grads[i]) and
 * out[i] <- alpha * sum_k avg_p[k] avg_q[k]^T, for the compressed tensors i (per-tensor
 * destination pointers; reference mem.data[:] = tensor - out, out.data[:] = p q^T). */
int psgd_reconstruct(psgd_plan* plan, void* const* grads, void* const* resid_out, void* const* out,
                     int32_t nterms, const float* const* term_p, const float* const* term_q,
                     const float* const* avg_p, const float* const* avg_q, float alpha, void* stream);

/* ------------------------------------ multi-GPU step with RCCL on the caller's stream ------ */
/* One process per GPU (reference: torch.distributed default group, powersgd.py:204-209 and
 * utils.py:43-49). The library drives RCCL itself, on the same stream as its kernels, so a
 * whole world-size-W step is ONE call with no host synchronisation and no per-collective
 * round trip through the host language. RCCL is resolved at run time (dlopen; an already loaded
 * librccl, e.g. PyTorch's, is reused): no link-time dependency.
 *   psgd_comm_unique_id  on rank 0: the communicator id (psgd_comm_id_bytes bytes), which the
 *                        caller broadcasts to every rank (e.g. torch.distributed);
 *   psgd_comm_init       on every rank, collectively: a communicator of `world` ranks on `device`.
 * psgd_aggregate_comm: PowerSGD.aggregate at world size W (reference :64-74 with
 * is_distributed()): for every power iteration the codec kernels and an in-place SUM all-reduce
 * of the out-factor state buffer (:204-209; the last iteration's collective grouped with the
 * SUM all-reduce of the uncompressed tensors packed /W into flat_out, utils.py:43-47), then the
 * output pass (alpha = 1/W). flat may be null (no uncompressed tensors). The whole plan is
 * one bucket here: a bucketed form (collectives on a second stream, event-ordered) was measured
 * host-enqueue-bound and removed. A poisoned communicator (an earlier failure)
 * is refused before anything is launched. */
int psgd_comm_id_bytes(int64_t* bytes);
int psgd_comm_unique_id(void* id_out);
int psgd_comm_init(int32_t world, int32_t rank, const void* id, int32_t device, psgd_comm** out);
int psgd_comm_destroy(psgd_comm* comm);
int psgd_aggregate_comm(psgd_plan* plan, void* const* grads, void* out, int64_t step, psgd_flat* flat,
                        void* const* unc, void* flat_out, psgd_comm* comm, void* stream);

/* ------------------------------------------ uncompressed tensors: flat average ------ */
/* AllReduce.aggregate minus the collective: flat[off_i + e] = x_i[e] / world_size (exact
 * copy when world_size == 1), then x_i[e] = 0. The caller SUM-all-reduces `flat` and
 * returns views of it (reference powersgd.py:22-31). Offsets are dense (torch.cat). */
int psgd_flat_create(const int64_t* numels, int32_t count, int32_t dtype, psgd_flat** out);
int psgd_flat_destroy(psgd_flat* flat);
int psgd_flat_workspace_bytes(const psgd_flat* flat, int64_t* bytes);
int psgd_flat_bind(psgd_flat* flat, int32_t device, void* workspace);
int psgd_flat_pack(psgd_flat* flat, void* const* tensors, void* flat_out, int32_t world_size,
                   void* stream);

/* PowerSGD.aggregate at world size 1 in one call (reference powersgd.py:64-74): the codec
 * step of psgd_aggregate on the compressed tensors `grads`, and the flat pack of the
 * uncompressed tensors `unc` into `flat_out` (psgd_flat_pack with world size 1) folded into
 * the codec's final-pass launch as extra workgroups (no launch of its own). Falls back to
 * two separate calls when the flat plan's dtype or device differs from the codec's. */
int psgd_aggregate_flat(psgd_plan* plan, void* const* grads, void* out, int64_t step, psgd_flat* flat,
                        void* const* unc, void* flat_out, void* stream);

/* ------------------------------------------ DDP bucket <-> parameter tensors ------ */
/* A run table maps a DDP bucket's flat buffer onto per-parameter tensors: run k covers
 * len[k] elements, bucket[bucket_off[k] + e] <-> tensors[tensor[k]][tensor_off[k] + e]. 64-bit
 * offsets throughout (no limit on the model's element count). `tensors` at call time is a host
 * array of ntensors device pointers (uploaded on the stream when it changes, like the codec's
 * gradient tables). psgd_runs_add: tensors += bucket (the error-feedback add, in the tensors'
 * dtype: fp32 / bf16 round to nearest even / fp64); psgd_runs_gather: bucket = tensors.
 * Runs must not overlap in the tensors (add) or in the bucket (gather). */
int psgd_runs_create(const int64_t* bucket_off, const int32_t* tensor, const int64_t* tensor_off,
                     const int64_t* len, int32_t nruns, int32_t ntensors, int32_t dtype, psgd_runs** out);
int psgd_runs_destroy(psgd_runs* runs);
int psgd_runs_workspace_bytes(const psgd_runs* runs, int64_t* bytes);
int psgd_runs_bind(psgd_runs* runs, int32_t device, void* workspace);
int psgd_runs_add(psgd_runs* runs, const void* bucket, void* const* tensors, void* stream);
int psgd_runs_gather(psgd_runs* runs, void* bucket, void* const* tensors, void* stream);

/* Run tables whose two sides differ: a bucket-side dtype and a tensor-side dtype, and optionally
 * a bucket side made of separate tensors. Accepted pairs: the three equal pairs (then exactly
 * psgd_runs_create) and (bucket PSGD_BF16, tensors PSGD_F32): an fp32 error-feedback residual fed
 * by bf16 gradients. Any other pair: PSGD_ERR_DTYPE. For the mixed pair
 *   add:    tensors[..] = tensors[..] + float(bucket[..])   exact upcast, ONE fp32 add, nothing is
 *                                                            rounded to bf16
 *   gather: bucket[..]  = bf16(tensors[..])                 round to nearest even
 * `source` null: the bucket side is one buffer; the table is driven by psgd_runs_add /
 * psgd_runs_gather as above (a DDP bucket). `source` given (nruns indices below nsources): run k's
 * bucket side is sources[source[k]] + bucket_off[k], `sources` a host array of nsources device
 * pointers passed at call time and uploaded when it changes, like `tensors` (the optimizer_step
 * flow, whose "bucket" is the caller's separate gradient tensors); such a table is driven by
 * psgd_runs_add_list / psgd_runs_gather_list. zero_source != 0: the add also stores +0.0 to every
 * source element it read (the gradients are consumed in the pass that reads them). One launch per
 * call, 2-byte / 4-byte alignment of the two sides independently. Calling the form the table was
 * not created for is PSGD_ERR_STATE. The workspace (psgd_runs_workspace_bytes) holds both pointer
 * tables. */
int psgd_runs_create_mixed(const int64_t* bucket_off, const int32_t* tensor, const int64_t* tensor_off,
                           const int64_t* len, const int32_t* source, int32_t nruns, int32_t ntensors,
                           int32_t nsources, int32_t bucket_dtype, int32_t tensor_dtype, psgd_runs** out);
int psgd_runs_add_list(psgd_runs* runs, void* const* sources, void* const* tensors, int32_t zero_source,
                       void* stream);
int psgd_runs_gather_list(psgd_runs* runs, void* const* sources, void* const* tensors, void* stream);

/* ------------------- fp32 error-feedback residual of bf16 gradients, in one call (W = 1) ------ */
/* The optimizer_step flow with the residual kept in fp32 (powersgd_amd/residual.py) is three
 * stages: the run-table ADD above (residual += float(g), g = +0.0), psgd_aggregate[_flat] on the
 * fp32 residual, and the run-table GATHER of the fp32 averages into bf16. psgd_aggregate_mixed is
 * DEFINED as exactly that sequence, and equals it bit for bit:
 *   1. residual[i][j] += float(grads_bf16[i][j])   one fp32 add per element
 *   2. grads_bf16[i][j] = +0.0
 *   3. psgd_aggregate(plan, residual, avg, step)
 *   4. out_bf16[j] = bf16(avg[j])                   round to nearest even
 * but the two element-wise stages run inside the codec's own gradient passes where they can:
 *   output fold  the step's final pass (k_final_proj / k_final_odd / k_apply) stores its output as
 *                bf16; the residual stays fp32. Every step of an eligible plan. At rank buckets 16
 *                and 32 that pass is k_apply's matrix-core tile (and its VALU fallback wherever
 *                k_apply<float> takes it: the choice follows the residual's alignment and the
 *                plan's output offset, never the bf16 buffer).
 *   ingest fold  the single-pass k_final_odd (num_iters_per_step = 1 on an odd step, ranks 1 and
 *                2: the step's only gradient pass) loads residual + float(g) and stores +0.0 to g
 *                beside its own residual. On every other step the library launches the run-table
 *                ADD itself, first (the same fold in k_even was measured slower than that ADD and
 *                is not kept; the odd-even pass and the unfused odd product have none).
 * `plan`: a bound PSGD_F32 plan driven at world size 1, rank bucket 1, 2, 4, 16 or 32 (largest
 * effective rank 1-4 or 9-32), one bucket; `residual[i]`: its fp32 tensors (the plan's gradients: alignment as for
 * psgd_aggregate); `grads_bf16[i]`: the fresh bf16 gradients, the plan's shapes, 2-byte aligned
 * (8-byte aligned tensors of m % 4 == 0 matrices take vector accesses); `out_bf16`: a dense bf16
 * buffer, 16-byte aligned, tensor i at element offset psgd_plan_output_offset(i). Any other plan
 * (rank bucket 8, wide: ranks above 32, fp64 or bf16 dtype, more than one bucket): PSGD_ERR_VALUE before
 * anything is launched, and psgd_plan_mixed_folds reports 0 / 0.
 * Every mixed kernel instance is admitted like the fused final pass (at least two waves per SIMD,
 * no scratch; asked of the runtime). Without an admitted ingest instance that fold is dropped (the
 * ADD launch takes its place); a plan whose final pass has no admitted bf16-output instance is
 * ineligible (there is no fp32 output buffer to fall back to).
 * psgd_plan_mixed_folds: which folds `step` takes (1 / 0 each). On an unbound plan the answer is
 * this build's on the current device (0 / 0 without one).
 * psgd_aggregate_mixed_flat: with the uncompressed tensors of psgd_aggregate_flat riding in the
 * final launch: `flat` an fp32 flat plan over their fp32 residual tensors `unc_residual`,
 * `unc_bf16` their bf16 gradients, `flat_out_bf16` the dense bf16 flat buffer: per element
 * flat = bf16(x + float(g)), x = +0.0, g = +0.0 (the ADD, the flat pack and the GATHER of the
 * three-stage flow). flat null or empty: psgd_aggregate_mixed.
 * The first mixed call (or fold query) of a bound plan makes one small device allocation owned by
 * the plan (pointer tables of the bf16 gradients, the ADD's run items), freed with the plan; the
 * caller's workspace layout is untouched. */
int psgd_aggregate_mixed(psgd_plan* plan, void* const* grads_bf16, void* const* residual,
                         void* out_bf16, int64_t step, void* stream);
int psgd_aggregate_mixed_flat(psgd_plan* plan, void* const* grads_bf16, void* const* residual,
                              void* out_bf16, int64_t step, psgd_flat* flat, void* const* unc_bf16,
                              void* const* unc_residual, void* flat_out_bf16, void* stream);
int psgd_plan_mixed_folds(const psgd_plan* plan, int64_t step, int32_t* fold_in, int32_t* fold_out);

/* ------------------- ... at world size W over a communicator, in one call ---------------------- */
/* The mixed form of psgd_aggregate_comm. DEFINED as this sequence, and equal to it bit for bit,
 * with nothing else observable:
 *   1. residual[i][j] += float(grads_bf16[i][j]), grads_bf16[i][j] = +0.0; the uncompressed
 *      tensors likewise: unc_residual += float(unc_bf16), unc_bf16 = +0.0
 *   2. psgd_aggregate_comm(plan, residual, avg_f32, step, flat, unc_residual, flat_f32, comm): the
 *      same kernels, the same collectives in the same order and the same count (num_iters_per_step
 *      all-reduces; the flat tail holds x / W and is grouped with the last factor's)
 *   3. out_bf16 = bf16(avg_f32), flat_out_bf16 = bf16(flat_f32)   round to nearest even
 * Where the stages run:
 *   output fold  every step: the final pass of the W > 1 sequence stores its output as bf16, the
 *                residual stays fp32. That pass is k_apply with two term sets (the residual from
 *                the local factors, the output alpha x the all-reduced ones), or, on steps whose
 *                last iteration is odd on a plan with the K-term fused final pass (rank buckets 1
 *                and 2), the output pass k_lowrank_out that follows k_final_odd. With a 1-rank
 *                communicator the two-term-set pass is the world-size-1 instance of
 *                psgd_aggregate_mixed.
 *   ingest       never folded (fold_in is 0): the library launches the run-table ADD first. The
 *                W > 1 sequence has no single-pass kernel to fold it into.
 *   flat tail    the all-reduce sums fp32 values, so the tail is staged in an fp32 buffer of
 *                flat->total floats owned by the plan (made or grown by the first call that needs
 *                it): stage = (x + float(g)) / W, x = g = +0.0 in a launch of its own before the
 *                first collective; flat_out_bf16 = bf16(stage) in the leading workgroups of the
 *                final launch (a launch of its own after the world-size-1 instance).
 * Arguments as psgd_aggregate_mixed_flat (flat null or empty: no uncompressed tensors) and
 * psgd_aggregate_comm. Eligible: a bound PSGD_F32 plan, rank bucket 1, 2, 4, 16 or 32 (not 8), not
 * wide, one bucket, whose final-pass instance of BOTH step parities is admitted (at least two waves per SIMD,
 * no scratch; asked of the runtime) for the communicator's world size. Anything else:
 * PSGD_ERR_VALUE before anything is launched or any collective issued, the communicator stays
 * usable, and psgd_plan_mixed_folds_comm reports 0 / 0. A poisoned communicator is refused at
 * entry (PSGD_ERR_STATE); any other failure past the argument checks poisons it, as in
 * psgd_aggregate_comm.
 * psgd_plan_mixed_folds_comm: the folds of `step` at world size `world` (>= 1): fold_in always 0,
 * fold_out 1 for an eligible plan. On an unbound plan the answer is this build's on the current
 * device (0 / 0 without one). */
int psgd_aggregate_mixed_comm(psgd_plan* plan, void* const* grads_bf16, void* const* residual,
                              void* out_bf16, int64_t step, psgd_flat* flat, void* const* unc_bf16,
                              void* const* unc_residual, void* flat_out_bf16, psgd_comm* comm,
                              void* stream);
int psgd_plan_mixed_folds_comm(const psgd_plan* plan, int64_t step, int32_t world,
                               int32_t* fold_in, int32_t* fold_out);

/* ------------------- ... with the averages stored at per-tensor destinations (DDP hook) -------- */
/* The completion of the DDP communication hook with an fp32 residual of bf16 gradients. The hook
 * adds every bucket into the residual when it arrives, so `residual` already holds residual +
 * gradients: this call runs NO ADD and takes no bf16 source. DEFINED as this sequence, and equal
 * to it bit for bit, with nothing else observable:
 *   1. psgd_aggregate_comm(plan, residual, avg_f32, step, flat, unc_residual, flat_f32, comm): the
 *      same kernels, collectives (order and count), residual, P/Q state and step semantics
 *   2. dst_bf16[i][j] = bf16(avg_f32 of tensor i [j]), unc_dst_bf16[k][j] = bf16(flat_f32 of
 *      tensor k [j])   round to nearest even
 * dst_bf16 is in the plan's tensor order, unc_dst_bf16 in the flat plan's. Each pointer is 2-byte
 * aligned or better (a parameter's view inside a DDP bucket, where parameters sit back to back)
 * and addresses numel dense bf16 elements; nothing outside those numel elements is written. They
 * are written, never accumulated into.
 * Where the stages run: the final pass of the communicator sequence (as in
 * psgd_aggregate_mixed_comm: k_apply with two term sets, k_lowrank_out after a fused k_final_odd,
 * the world-size-1 k_apply for a 1-rank communicator) stores the bf16 rounding itself, at
 * dst_bf16[tensor]. Its tiles, loads and arithmetic are laid out from the residual's alignment
 * and the plan's offsets exactly as in step 1; only the store follows the destination: a vector
 * tile whose destination (tensor base + row offset) is 8-byte aligned stores 8 bytes, any other
 * four 2-byte elements, chosen once per tile; every store goes through a descriptor that spans
 * the tile's rows of its own tensor. The flat tail is packed into the plan's fp32 staging buffer
 * where psgd_aggregate_comm packs (stage = x / W, x = +0.0), all-reduced there, and rounded into
 * unc_dst_bf16 by the leading workgroups of the final launch (a launch of its own after the
 * world-size-1 instance).
 * Eligibility, refusals and poisoning are exactly those of psgd_aggregate_mixed_comm, with the
 * admission asked for the destination-table instances themselves. psgd_plan_mixed_folds_dst:
 * fold_out 1 where the call would run at world size `world` (>= 1), 0 for an ineligible plan. */
int psgd_aggregate_mixed_comm_dst(psgd_plan* plan, void* const* residual, void* const* dst_bf16,
                                  int64_t step, psgd_flat* flat, void* const* unc_residual,
                                  void* const* unc_dst_bf16, psgd_comm* comm, void* stream);
int psgd_plan_mixed_folds_dst(const psgd_plan* plan, int64_t step, int32_t world, int32_t* fold_out);

/* ------------------- ... over the IPC exchange (psgd_ipc_*), in one call ----------------------- */
/* The mixed forms of psgd_aggregate_ipc: world size W over the plan's open exchange session, no
 * communicator, no host barrier. Each is DEFINED as a sequence of existing calls and equal to it
 * bit for bit, with nothing else observable.
 * psgd_aggregate_mixed_ipc (arguments as psgd_aggregate_mixed_comm without the communicator):
 *   1. residual[i][j] += float(grads_bf16[i][j]), grads_bf16[i][j] = +0.0; the uncompressed
 *      tensors likewise: unc_residual += float(unc_bf16), unc_bf16 = +0.0
 *   2. psgd_aggregate_ipc(plan, residual, avg_f32, step, flat, unc_residual, flat_f32): the same
 *      kernels, the same exchanges with the same flags and epochs
 *   3. out_bf16 = bf16(avg_f32), flat_out_bf16 = bf16(flat_f32)   round to nearest even
 * psgd_aggregate_mixed_ipc_dst (arguments as psgd_aggregate_mixed_comm_dst without the
 * communicator; `residual` already holds residual + gradients, NO ADD, no dense output):
 *   1. psgd_aggregate_ipc(plan, residual, avg_f32, step, flat, unc_residual, flat_f32)
 *   2. dst_bf16[i][j] = bf16(avg_f32 of tensor i [j]), unc_dst_bf16[k][j] = bf16(flat_f32 of
 *      tensor k [j]); nothing outside a destination's numel elements is written
 * Where the stages run:
 *   ingest       never folded: the dense form launches the run-table ADD first.
 *   flat tail    packed straight into this rank's last exchange slot (dense form: slot = (x +
 *                float(g)) / W, x = g = +0.0 in a launch of its own; _dst form: slot = x / W,
 *                x = +0.0 where psgd_aggregate_ipc packs, inside the first even product's launch
 *                on steps that start even). The LAST exchange sums the W slots' flat regions per
 *                flat item in rank order and stores bf16(sum) at flat_out_bf16 / unc_dst_bf16
 *                itself (k_xchg_mix): no fp32 staging buffer, no fp32 copy of the flat sums, no
 *                round pass. A step without uncompressed tensors launches k_xchg alone.
 *   output fold  every step: the output pass after the exchanges stores bf16 (the instances of
 *                psgd_aggregate_mixed_comm / _comm_dst: k_apply with two term sets, k_lowrank_out
 *                after a fused k_final_odd, the world-size-1 k_apply in a 1-rank session).
 * Eligible: as psgd_aggregate_mixed_comm / _comm_dst (a bound PSGD_F32 plan, rank bucket 1, 2, 4,
 * 16 or 32, not wide, one bucket, the final-pass instance of BOTH step parities admitted for the
 * session's world size: psgd_plan_mixed_folds_comm / psgd_plan_mixed_folds_dst answer for it), with
 * an open exchange session (psgd_ipc_open), flat->total within the session's flat_numel,
 * step < 2^32 - 1 and no timed-out wait pending. An ineligible plan, an oversized flat plan, an
 * out-of-range step and a null pointer: PSGD_ERR_VALUE; no session, or a timed-out wait
 * (psgd_ipc_status): PSGD_ERR_STATE. The argument errors (a null argument, step < 0) are reported
 * before the plan's state (an unbound plan: PSGD_ERR_STATE), then the plan's eligibility, then the
 * session's state. Every refusal comes before anything is launched: gradients,
 * residual and P/Q state stay as they were and the session stays usable. After a wait of this call
 * times out, its bf16 outputs (flat tail included) hold NaN, as psgd_aggregate_ipc's fp32 ones. */
int psgd_aggregate_mixed_ipc(psgd_plan* plan, void* const* grads_bf16, void* const* residual,
                             void* out_bf16, int64_t step, psgd_flat* flat, void* const* unc_bf16,
                             void* const* unc_residual, void* flat_out_bf16, void* stream);
int psgd_aggregate_mixed_ipc_dst(psgd_plan* plan, void* const* residual, void* const* dst_bf16,
                                 int64_t step, psgd_flat* flat, void* const* unc_residual,
                                 void* const* unc_dst_bf16, void* stream);

/* ------------- the default (fp32) DDP hook's one-call completion: fp32 destinations ------------ */
/* psgd_aggregate_comm and psgd_aggregate_ipc with every average stored at its tensor's own
 * destination (the tensor's gradient view inside a DDP bucket) instead of an output slab that a
 * per-bucket psgd_runs_gather then copies. Each is DEFINED as a sequence of existing calls and
 * equal to it bit for bit, with nothing else observable.
 * psgd_aggregate_comm_dst:
 *   1. psgd_aggregate_comm(plan, grads, out, step, flat, unc, flat_out, comm): the same kernels in
 *      the same order, the same collectives (order and count), residual and P/Q state
 *   2. dst[i][e] = out_i[e], unc_dst[k][e] = flat_k[e]
 * psgd_aggregate_ipc_dst: the same with psgd_aggregate_ipc (the same exchanges, flags and epochs).
 * dst is in the plan's tensor order, unc_dst in the flat plan's. Each pointer is 4-byte aligned or
 * better and addresses numel dense fp32 elements; nothing outside those numel elements is
 * written. They are written, never accumulated into.
 * Where the stages run: the final pass of the sequence (k_apply with two term sets; k_apply's
 * world-size-1 form for one rank; k_lowrank_out after a fused k_final_odd; the VALU tiles at rank
 * buckets 1-8, the matrix-core tiles at 16 and 32) is its destination-table instance. Its tiles,
 * loads and arithmetic are laid out from the gradients' alignment and the plan's offsets exactly
 * as in step 1; only the output store follows the destination: a vector tile whose first
 * destination element is 16-byte aligned stores 16 bytes, any other four 4-byte elements, chosen
 * once per tile; every store goes through a descriptor that spans the tile's rows of its own
 * tensor. The flat tail is packed into a staging buffer of the plan's own (flat->total floats)
 * where psgd_aggregate_comm / _ipc pack into flat_out, summed there by the collective / the last
 * exchange, and copied to unc_dst by the leading workgroups of the final launch.
 * Eligible: a bound PSGD_F32 plan, not wide (rank buckets 1-32), one bucket, with EVERY
 * destination-table instance its routes name admitted (at least two waves per SIMD, no scratch;
 * both step parities, one rank and W > 1). psgd_plan_dst_ok: *ok = 1 for such a plan, else 0: a
 * property of the plan (step >= 0 and world >= 1 are validated only).
 * Refusals: a non-fp32 plan PSGD_ERR_DTYPE; a wide plan, more than one bucket, an instance that
 * is not admitted, a null pointer, a flat plan that is not fp32 on the codec's device, flat->total
 * above the session's flat_numel: PSGD_ERR_VALUE; a destination that is not 4-byte aligned:
 * PSGD_ERR_LAYOUT; an unbound plan, a poisoned communicator, no open session or a timed-out wait:
 * PSGD_ERR_STATE. Every refusal comes before any launch, collective or exchange: gradients,
 * destinations and P/Q state stay as they were, and the communicator / session stays usable. */
int psgd_aggregate_comm_dst(psgd_plan* plan, void* const* grads, void* const* dst, int64_t step,
                            psgd_flat* flat, void* const* unc, void* const* unc_dst, psgd_comm* comm,
                            void* stream);
int psgd_aggregate_ipc_dst(psgd_plan* plan, void* const* grads, void* const* dst, int64_t step,
                           psgd_flat* flat, void* const* unc, void* const* unc_dst, void* stream);
int psgd_plan_dst_ok(const psgd_plan* plan, int64_t step, int32_t world, int32_t* ok);

/* ------------------------ global-norm clipping of a step's averages (clip_grad_norm_) ---------- */
/* torch.nn.utils.clip_grad_norm_ (L2) over everything a step returned, on the stream, with no host
 * synchronisation: norm = sqrt(sum of squares of the compressed averages `out` and of the dense
 * uncompressed averages `flat_out`), coef = min(1, max_norm / (norm + 1e-6)), and, when coef < 1,
 * every element x <- x * float(coef) (bf16: bf16(float(x) * float(coef)), round to nearest even;
 * fp64: x * coef). All sums are fp64 in a fixed order: the same inputs give the same bits.
 *   `out`       the compressed averages of `step` (the output buffer the step wrote; the plan's
 *               dtype, psgd_plan_output_numel elements); NULL: none (a warm-up step)
 *   `flat_out`  the dense uncompressed averages (the plan's dtype), flat_numel elements; NULL / 0: none
 *   `max_norm`  > 0; +inf: the norm only, no scale launch. <= 0 or NaN: PSGD_ERR_VALUE
 *   `result`    device, 2 doubles, 8-byte aligned: norm, coef. A non-finite norm gives coef = NaN
 *               and leaves every output untouched. The scale pass reads coef from here on the
 *               device; its workgroups return at once when coef >= 1
 *   `form`      how the compressed tensors' sum of squares is formed:
 *     1 factors a compressed tensor's average is A = alpha sum_k P_k Q_k^T over the term set the
 *               step's output pass read; with the terms stacked, P^ = [P_0 .. P_{I-1}] and Q^
 *               likewise, ||A||_F^2 = alpha^2 <P^^T P^, Q^^T Q^>_F exactly (the cross blocks
 *               between iterations included): two small fp64 Gram matrices per matrix, read from
 *               the factors; the n x m output is never read. The plan records the term set when a
 *               whole-plan output pass runs (psgd_decompress, every psgd_aggregate* form); the call
 *               must follow the aggregate / decompress of `step` at world size `world` on the same
 *               stream, before the plan's next psgd_compress. Refused before any launch where it
 *               does not apply: a wide plan (ranks above 32), an fp64 plan, num_iters_per_step x
 *               rank bucket > 64, or `out` NULL: PSGD_ERR_VALUE; no record of (`step`, `world`)
 *               (never run, run per bucket, the next step already started, the plan re-bound):
 *               PSGD_ERR_STATE.
 *     2 stream  a sum of squares over `out` (one read of the outputs).
 *     0 auto    factors where they apply, else stream (psgd_plan_norm_form reports which;
 *               PSGD_NORM_FORM=auto|factors|stream, read at psgd_plan_create, overrides the choice
 *               for A/B runs, the factor form still only where it applies).
 * `flat_out` always takes the stream form. The first call makes one device allocation owned by the
 * plan (work items, Gram partials, per-workgroup partials), freed with it; the caller's workspace
 * layout is untouched. An unbound plan: PSGD_ERR_STATE; a buffer not aligned to its element size
 * (`result`: 8 bytes): PSGD_ERR_LAYOUT.
 * psgd_plan_norm_form: the form auto takes for (`step`, `world`): 1 or 2. On an unbound plan the
 * answer is the plan's own (no step has run: 1 wherever the factor form can apply). */
int psgd_clip_outputs(psgd_plan* plan, int64_t step, int32_t world, void* out, void* flat_out,
                      int64_t flat_numel, double max_norm, int32_t form, double* result, void* stream);
int psgd_plan_norm_form(const psgd_plan* plan, int64_t step, int32_t world, int32_t* form);

/* psgd_clip_dst: psgd_clip_outputs for the direct-store completion (psgd_aggregate_comm_dst /
 * psgd_aggregate_ipc_dst), whose averages lie at per-tensor destinations and in no slab. Called
 * right after that step on the same stream with the same `dst`, `flat` and `unc_dst`. DEFINED as,
 * and bit for bit equal to (result[0..1], every destination element, nothing outside the
 * destinations' numel elements), this sequence, which is never run:
 *   1. copy every dst[i] / unc_dst[k] into a dense output slab (the plan's output offsets) / a
 *      dense flat slab (the flat plan's order), each the base of an allocation of its own
 *   2. psgd_clip_outputs(plan, step, world, out, flat_out, flat->total, max_norm, form = 1, result)
 *   3. copy back
 * Why the bits agree. Compressed tensors: the factor form reads the plan's recorded term set,
 * which the destination-table output pass records exactly as the slab one does; the n x m
 * averages are never read, so where they lie does not matter. Uncompressed tensors: the stream sum
 * runs over the plan's own fp32 staging buffer (flat->total floats), which still holds the sums
 * that the step's copy items wrote to unc_dst, in the flat plan's layout. That buffer is the base
 * of an allocation, like the flat slab of step 1, so the sum's split into head, 16-byte vectors
 * and tail and its workgroup partition (functions of the base's alignment and the length alone)
 * are the same, and so is every partial sum. The scale is element-wise (x * float(coef)), so its
 * partition cannot show. There is no stream form for the compressed tensors: a sum over scattered
 * destinations would partition differently from the slab's.
 * The scale pass (k_norm_scale_dst, fp32) goes through the two destination tables in work items
 * built once per plan / flat plan from the numels; a destination needs 4-byte alignment only (an
 * item splits into a head of 0-3 elements, 16-byte vectors and a tail by its pointer). Its
 * workgroups return at once, writing nothing, unless coef < 1 and the norm is finite.
 * max_norm = +inf: the norm only, no scale launch.
 * psgd_plan_clip_dst_ok: *ok = 1 exactly when the plan is one psgd_plan_dst_ok can serve by shape
 * (PSGD_F32, not wide, one bucket), num_iters_per_step x rank bucket <= 64, and PSGD_NORM_FORM does
 * not force the stream form. No device is asked.
 * Refusals, all before any launch: a null plan / dst / result, a flat plan with total > 0 and a
 * null unc_dst or a null entry, max_norm <= 0 or NaN, a plan for which psgd_plan_clip_dst_ok is 0:
 * PSGD_ERR_VALUE; a destination that is not 4-byte aligned, `result` not 8-byte aligned:
 * PSGD_ERR_LAYOUT; an unbound plan, no record of (`step`, `world`), a flat tail with no staging of
 * at least flat->total floats from a preceding direct-store call: PSGD_ERR_STATE. */
int psgd_clip_dst(psgd_plan* plan, int64_t step, int32_t world, void* const* dst, psgd_flat* flat,
                  void* const* unc_dst, double max_norm, double* result, void* stream);
int psgd_plan_clip_dst_ok(const psgd_plan* plan, int32_t* ok);

/* ------------------------ skipping a non-finite step on the device ----------------------------- */
/* psgd_guard_outputs: called last after a step (and after its psgd_clip_outputs, never before: the
 * clip's factor form reads the factors this call may reset) on the same stream. Two launches, no
 * host synchronisation. k_guard_check scans, for an all-ones exponent field (NaN, +inf, -inf),
 *   - the plan's bound P state and Q state, psgd_plan_factor_numel elements each (fp32; fp64 on
 *     PSGD_F64 plans): the gradient enters every product of every iteration, so NaN * x, inf * 0 and
 *     inf - inf of a non-finite gradient element all land in the out-factor the step leaves there;
 *     at world size W the factors are all-reduced, so every rank reads the same bits;
 *   - `flat_out`, the dense uncompressed averages (the plan's dtype), flat_numel elements;
 * and raises one flag word with an integer atomic max (order-independent). k_guard_apply reads the
 * word. A finite step: every workgroup returns at once and nothing but result[0] = 0 is written.
 * Otherwise the step is SKIPPED:
 *   - every compressed gradient tensor grads[i] (the plan's shapes and dtype; they hold the
 *     error-feedback residual by now) becomes all-zero bits: exactly its numel elements, a tensor
 *     needs element alignment only (work items built once per plan split into a head, 16-byte
 *     vectors and a tail by the item's pointer);
 *   - `out` (psgd_plan_output_numel elements) and `flat_out` become all-zero bits;
 *   - P <- p_init and Q <- q_init (psgd_plan_factor_numel elements of the factors' type each), bit
 *     for bit: with the retained initial draw the codec is a freshly constructed one;
 *   - result[0] = 1 and result[1] += 1.
 * The uncompressed INPUTS are not touched: the step itself has zeroed them (psgd_flat_pack).
 *   `out`       non-NULL: a compressing step; grads, p_init and q_init are required.
 *               NULL: a warm-up step; only `flat_out` is scanned and zeroed, P and Q are neither read
 *               nor reset, `grads` is ignored
 *   `flat_out`  NULL / flat_numel 0: none
 *   `result`    device, 2 x int64, 8-byte aligned: [0] this call skipped (0 or 1, rewritten by every
 *               call), [1] the running count (the caller zeroes it once)
 * Serves every plan: every rank bucket, wide plans, PSGD_F32 / PSGD_BF16 / PSGD_F64; it needs no
 * recorded term set. The first call makes one device allocation owned by the plan (the flag word,
 * the work items, the change-detected gradient pointer tables), freed with it; the caller's
 * workspace layout is untouched. Not covered: finite inputs whose residual arithmetic overflows
 * while the factors stay finite.
 * Refusals, all before any launch: a null plan / result, a compressing call with a null grads /
 * grads[i] / p_init / q_init, flat_numel < 0 or > 0 with a null flat_out: PSGD_ERR_VALUE; a buffer
 * or gradient not aligned to its element size, `result` not 8-byte aligned: PSGD_ERR_LAYOUT; an
 * unbound plan: PSGD_ERR_STATE. */
int psgd_guard_outputs(psgd_plan* plan, void* const* grads, void* out, void* flat_out, int64_t flat_numel,
                       const void* p_init, const void* q_init, int64_t* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_H */
