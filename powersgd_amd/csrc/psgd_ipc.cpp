// All-reduce over HIP IPC (psgd_ipc_*, psgd_aggregate_ipc; include/psgd.h): the process-lifetime
// exchange arena, the exchange sessions of a plan (psgd_ipc_create; psgd_ipc_create2, which also
// serves wide plans and their two-shot exchange) and the step driver.
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>

#include "psgd_plan.h"

namespace {

// ---------------------------------------------------- process-lifetime IPC exchange arena ---
// Exchange buffers of the one-shot all-reduce (psgd_ipc_*) are REGIONS of per-device chunks that
// this process allocates once and never frees, and every peer chunk is mapped once per process
// and never unmapped (round 6). A session (psgd_ipc_create .. psgd_ipc_close) takes a region,
// zeroes its header and draws a fresh nonce; a later session of the same size gets the same
// region back. There is no hipFree -> hipMalloc -> hipIpcOpenMemHandle cycle between two
// sessions of one process, so a peer can never be handed a mapping of a freed buffer (the
// round-5 r05a-new mismatch: the second same-size session after a closed one read stale sums,
// which a cached mapping of the first session's freed allocation, whose flags still carried
// higher epochs than the new session's, produces exactly). The nonce check at open and the
// nonce-tagged flags stay as guards.
struct XchgChunk {
    int device = -1;
    char* base = nullptr;
    size_t bytes = 0;
    hipIpcMemHandle_t handle{};
};

class XchgArena {
  public:
    static constexpr size_t kAlign = 4096;
    static constexpr size_t kMinChunk = size_t(64) << 20;

    // a region of at least `bytes` on `device`: first fit in a free range, else a new chunk
    int acquire(int device, size_t bytes, int* chunk, size_t* off) {
        std::lock_guard<std::mutex> lock(mu_);
        bytes = (bytes + kAlign - 1) & ~(kAlign - 1);
        for (size_t i = 0; i < free_.size(); ++i) {
            Range& f = free_[i];
            if (chunks_[size_t(f.chunk)].device != device || f.bytes < bytes) continue;
            *chunk = f.chunk;
            *off = f.off;
            f.off += bytes;
            f.bytes -= bytes;
            if (f.bytes == 0) free_.erase(free_.begin() + long(i));
            ++reuses_;
            return PSGD_OK;
        }
        XchgChunk c;
        c.device = device;
        c.bytes = std::max(kMinChunk, (bytes + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1));
        if (hipMalloc(reinterpret_cast<void**>(&c.base), c.bytes) != hipSuccess)
            return fail(PSGD_ERR_DEVICE, "hipMalloc of the IPC exchange arena failed");
        if (hipIpcGetMemHandle(&c.handle, c.base) != hipSuccess) {
            (void)hipFree(c.base);  // never exported: no peer can map it
            return fail(PSGD_ERR_DEVICE, "hipIpcGetMemHandle of the IPC exchange arena failed");
        }
        chunks_.push_back(c);
        ++allocs_;
        *chunk = int(chunks_.size()) - 1;
        *off = 0;
        if (c.bytes > bytes) free_.push_back(Range{*chunk, bytes, c.bytes - bytes});
        return PSGD_OK;
    }
    // give a region back (its bytes stay allocated and exported; adjacent free ranges merge)
    void release(int chunk, size_t off, size_t bytes) {
        std::lock_guard<std::mutex> lock(mu_);
        bytes = (bytes + kAlign - 1) & ~(kAlign - 1);
        Range r{chunk, off, bytes};
        for (size_t i = 0; i < free_.size();) {
            Range& f = free_[i];
            if (f.chunk == r.chunk && (f.off + f.bytes == r.off || r.off + r.bytes == f.off)) {
                r.off = std::min(r.off, f.off);
                r.bytes += f.bytes;
                free_.erase(free_.begin() + long(i));
                i = 0;
            } else {
                ++i;
            }
        }
        free_.push_back(r);
    }
    XchgChunk chunk(int i) {
        std::lock_guard<std::mutex> lock(mu_);
        return chunks_[size_t(i)];
    }
    // the process's mapping of a peer chunk: opened at the first session that needs it, kept
    // for the life of the process (the peer never frees the chunk either)
    int map_peer(int device, const hipIpcMemHandle_t& h, char** base) {
        std::lock_guard<std::mutex> lock(mu_);
        std::string key(reinterpret_cast<const char*>(&h), sizeof(h));
        key += std::to_string(device);
        auto it = peers_.find(key);
        if (it != peers_.end()) {
            *base = it->second;
            return PSGD_OK;
        }
        void* v = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&v, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return fail(PSGD_ERR_DEVICE, std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e));
        ++opens_;
        *base = static_cast<char*>(v);
        peers_.emplace(key, *base);
        return PSGD_OK;
    }
    void counters(int64_t* out) {
        std::lock_guard<std::mutex> lock(mu_);
        out[0] = allocs_;   // chunks allocated (hipMalloc) by this process
        out[1] = opens_;    // peer chunks mapped (hipIpcOpenMemHandle) by this process
        out[2] = reuses_;   // regions served from already-allocated chunks
        out[3] = 0;         // chunks freed: never
    }

  private:
    struct Range {
        int chunk;
        size_t off, bytes;
    };
    std::mutex mu_;
    std::vector<XchgChunk> chunks_;
    std::vector<Range> free_;
    std::map<std::string, char*> peers_;
    int64_t allocs_ = 0, opens_ = 0, reuses_ = 0;
};

XchgArena& xchg_arena() {
    static XchgArena* a = new XchgArena();  // never destroyed: chunks and mappings live to exit
    return *a;
}

// an exchange handle: the HIP IPC handle of the arena chunk, the region's byte offset in it,
// then the session nonce (last, 4 bytes)
constexpr size_t kHandleBytes = sizeof(hipIpcMemHandle_t) + sizeof(uint64_t) + sizeof(uint32_t);

}  // namespace

// (never freed, never unmapped: a peer's mapping stays valid; teardown is still collective,
// psgd_ipc_close + barrier, so that no peer kernel reads the region when a later session
// re-zeroes it)
void psgd::ipc_release(psgd_plan* p) {
    if (p->ipc_buf) xchg_arena().release(p->ipc_chunk, p->ipc_off, p->ipc_bytes);
    p->ipc_buf = nullptr;
}

int psgd::ipc_check(const psgd_plan* p, int64_t step) {
    if (p->ipc_peer.empty()) return fail(PSGD_ERR_STATE, "psgd_ipc_open first");
    // a wait of an earlier step gave up: that step's sums were invalid and the two-parity slot
    // reuse is no longer safe, so every later step is refused (the ranks have drifted apart)
    if (p->xerr_set())
        return fail(PSGD_ERR_STATE, "an earlier IPC exchange wait timed out (a peer did not arrive within "
                                    "PSGD_IPC_SPIN); the exchange is invalid until psgd_ipc_close");
    if (step < 0 || step >= 0xffffffffLL) return fail(PSGD_ERR_VALUE, "step out of range (epochs are 32-bit)");
    if (p->ipc_x2 && step >= 0x7fffffffLL)  // two epochs per step
        return fail(PSGD_ERR_VALUE, "step out of range (a psgd_ipc_create2 session of a wide plan takes step < 2^31 - 1)");
    return PSGD_OK;
}

// World size W over the IPC exchange (include/psgd.h): per iteration the codec kernels (the
// reduction or fused final pass also writes the local factor into this rank's exchange slot),
// then k_xchg (flag, bounded wait for the peers' flags, rank-order SUM into the state buffer; the
// last one also sums the uncompressed tensors packed /W into flat_out), then the output pass.
// Nothing leaves the stream: no host barrier, no host synchronisation.
// `mix` (psgd_aggregate_mixed_ipc): the flat tail is ingest-packed into the slot in a launch of its
// own first (flat_ingest_item, the slot as its stage), the last exchange is k_xchg_mix (the flat
// sums stored as bf16 into `flat_out`) and the output pass runs its bf16-output instance with no
// flat items. `mix` and `dst` (psgd_aggregate_mixed_ipc_dst): `grads` already holds residual +
// gradients, so the flat tail is packed as without `mix`, and both stores follow dst's tables.
// Every other launch, flag and epoch is the same in the three forms.
int psgd::aggregate_ipc_ctx(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f, void* const* unc,
                            void* flat_out, hipStream_t s, const MixArgs* mix, const MixDst* dst,
                            const DirectDst* fdst) {
    const bool has_flat = f != nullptr;
    const int world = p->ipc_world;
    const int last = p->iters - 1;
    static const uint32_t spin = uint32_t(std::min<int64_t>(env_int("PSGD_IPC_SPIN", int64_t(1) << 26), 0xffffffffLL));
    // x / W into this rank's last slot: inside the first even product's launch when the step
    // starts even, else its own launch
    FlatArgs fa{};
    const bool ingest = mix && !dst;
    const bool fold = has_flat && !ingest && p->even(step, 0) && !p->wide();  // wide products carry no flat pack
    float* flat_slot = p->xslot(step, last) + p->ipc_flat_off;
    if (has_flat) {
        if (int st = flat_args(f, unc, flat_slot, world, s, &fa)) return st;
        if (ingest) {
            MixArgs in = *mix;
            in.stage = flat_slot;  // its stores are write-through (kStAuxSlot), as the pack's
            PSGD_HIP(launch_flat_ingest(fa, in, s));
        } else if (!fold) {
            PSGD_HIP(launch_flat_pack(f->dtype, fa, s));
        }
    }
    StepCtx c;
    // rank 1: the joint group norm of every summed factor is folded as at world size 1 (no
    // k_orth_reg launch): k_xchg leaves per-item sums of squares and a raw copy (history slot 2)
    // that the next iteration's kernels normalise on the fly
    const bool nfold = c.fuse = p->rbucket == 1;
    c.raw_slot = 2;
    // ranks 2/4, two iterations (every step starts even): the Q orthonormalisation from the
    // exchange's Gram partials of the summed Q (k_orth_chain instead of k_orth_chol)
    const bool gfold = c.xgram = p->qfold_ok && p->iters == 2 && p->even(step, 0);
    c.fl = fold ? &fa : nullptr;
    for (int it = 0; it < p->iters; ++it) {
        c.xout = p->xslot(step, it);
        if (int st = compress_impl(p, grads, step, it, s, c)) return st;
        const bool e = p->even(step, it);
        XchgArgs xa{};
        const bool ss_out = nfold && it + 1 < p->iters;
        const bool gram = gfold && it == 0;  // even: the Q side; k_orth_chain of iteration 1 reads the Gram
        if (ss_out || gram) {  // per reduction item of the summed factor, and its raw copy
            xa.items = p->dev(e ? p->red_even : p->red_odd);
            xa.nitems = int32_t(e ? p->red_even.size() : p->red_odd.size());
            xa.mats = p->dev(p->mats);
            xa.even = e ? 1 : 0;
            xa.dst2 = p->hist(2, it);
            if (ss_out) xa.ss_out = p->dev<float>(p->o_ss) + size_t(it & 1) * p->ss_stride;
            if (gram) xa.gram = p->dev<double>(p->o_gram);
            if (gram) xa.gram_r = p->rbucket;
        }
        xa.peers = reinterpret_cast<const char* const*>(p->dev(p->ipc_peer));
        xa.own_flag = reinterpret_cast<uint64_t*>(p->ipc_buf) + it;
        xa.flag_off = int64_t(it) * int64_t(sizeof(uint64_t));
        xa.slot_off = p->xslot_off(step, it);
        xa.dst = e ? p->Q : p->P;
        xa.n = e ? p->qtot : p->ptot;
        const bool tail = it == last && has_flat;
        if (tail) {
            xa.flat_dst = mix ? nullptr : fdst ? fdst->stage : static_cast<float*>(flat_out);
            xa.flat_off = p->ipc_flat_off;
            xa.nflat = f->total;
        }
        // sessions of psgd_ipc_create2 on a wide plan: two epochs per step (psgd_plan::ipc_x2)
        xa.epoch = p->ipc_x2 ? 2 * (uint64_t(step) + 1) : uint64_t(step) + 1;
        xa.nonces = p->dev(p->ipc_nonces);
        xa.own_nonce = p->ipc_nonce;
        xa.spin_limit = spin;
        xa.world = world;
        xa.rank = p->ipc_rank;
        xa.err = p->xerr_dev;
        xa.err_dev = reinterpret_cast<int32_t*>(static_cast<char*>(p->ipc_buf) + kXchgErrOff);
        if (tail && mix) {  // the summed flat tail goes out as bf16 (the last iteration never takes the item form)
            XchgMixArgs xm{};
            xm.entries = fa.entries;
            xm.items = fa.items;
            xm.nitems = fa.nitems;
            xm.flat_out = dst ? nullptr : flat_out;
            xm.unc_dst = dst ? dst->unc_dst : nullptr;
            PSGD_HIP(launch_xchg_mix(xa, xm, dst != nullptr, s));
        } else if (p->ipc_two_shot(e ? 1 : 0)) {
            // reduce-scatter on the first epoch of the step, all-gather (and the flat tail) on the
            // second, as two launches: the kernel boundary drains the in-place shard stores
            XchgArgs rs = xa;
            rs.epoch = xa.epoch - 1;
            PSGD_HIP(launch_xchg_rs(rs, s));
            PSGD_HIP(launch_xchg_ag(xa, s));
        } else {
            PSGD_HIP(launch_xchg(xa, s));
        }
    }
    // the output pass: the route and the term sources are the same with and without `mix` (fuse and
    // write_out clear: the earlier iterations' summed factors in history slot 2, where the item form
    // of k_xchg or k_orth's save left them); no flat items ride in it
    StepCtx d = mix ? comm_out_ctx(mix, dst) : StepCtx{};
    if (fdst) {  // psgd_aggregate_ipc_dst: the last exchange summed the flat tail into fdst->stage; its
                 // copy items ride in the output pass's destination-table instance
        d.fdst = fdst;
        d.fl = has_flat ? &fa : nullptr;
    }
    return decompress_impl(p, grads, out, step, world, s, d);
}

extern "C" {

int psgd_ipc_handle_bytes(int64_t* bytes) {
    if (!bytes) return fail(PSGD_ERR_VALUE, "null argument");
    *bytes = int64_t(kHandleBytes);
    return PSGD_OK;
}

}  // extern "C"

namespace {

int64_t a64(int64_t x) { return (x + 63) & ~int64_t(63); }

// the session behind psgd_ipc_create and psgd_ipc_create2, after their argument checks
int ipc_create_checked(psgd_plan* p, int64_t flat_numel, void* handle_out) {
    if (!p->ipc_peer.empty()) return fail(PSGD_ERR_STATE, "exchange session open (psgd_ipc_close first)");
    DevScope scope(p->device);
    const int64_t flat_off = a64(std::max<int64_t>(p->fmax, 1));
    const int64_t slot = flat_off + a64(flat_numel);
    const size_t bytes = size_t(kXchgHeader) + size_t(2 * p->iters * slot) * sizeof(float);
    // a region of the process's arena: this plan's previous region when it is large enough (a
    // re-opened session), else a new one (the old one goes back to the arena)
    if (p->ipc_buf && p->ipc_bytes < bytes) ipc_release(p);
    if (!p->ipc_buf) {
        int chunk = -1;
        size_t off = 0;
        if (int st = xchg_arena().acquire(p->device, bytes, &chunk, &off)) return st;
        p->ipc_chunk = chunk;
        p->ipc_off = off;
        p->ipc_bytes = bytes;
        p->ipc_buf = xchg_arena().chunk(chunk).base + off;
    }
    p->ipc_flat_off = flat_off;
    p->ipc_flat_cap = flat_numel;
    p->ipc_slot = slot;
    PSGD_HIP(hipMemset(p->ipc_buf, 0, bytes));  // flags at epoch 0, error word clear
    if (!p->xerr_host) {
        PSGD_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->xerr_host), sizeof(int32_t),
                               hipHostMallocMapped | hipHostMallocCoherent));
        PSGD_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&p->xerr_dev), p->xerr_host, 0));
    }
    __atomic_store_n(p->xerr_host, 0, __ATOMIC_RELEASE);
    // a fresh session nonce (never 0: a zeroed header never matches), in the header and the handle
    {
        static std::atomic<uint32_t> counter{0};
        uint64_t z = uint64_t(std::chrono::steady_clock::now().time_since_epoch().count()) ^
                     (uint64_t(reinterpret_cast<uintptr_t>(p->ipc_buf)) << 7) ^ (uint64_t(getpid()) << 40) ^
                     (uint64_t(counter.fetch_add(1)) * 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        p->ipc_nonce = uint32_t(z ^ (z >> 31)) | 1u;
    }
    PSGD_HIP(hipMemcpy(p->ipc_buf + kXchgNonceOff, &p->ipc_nonce, sizeof(uint32_t), hipMemcpyHostToDevice));
    PSGD_HIP(hipDeviceSynchronize());  // zeroed before any peer can open and poll it
    const XchgChunk c = xchg_arena().chunk(p->ipc_chunk);
    char* h = static_cast<char*>(handle_out);
    const uint64_t off64 = uint64_t(p->ipc_off);
    std::memcpy(h, &c.handle, sizeof(hipIpcMemHandle_t));
    std::memcpy(h + sizeof(hipIpcMemHandle_t), &off64, sizeof(uint64_t));
    std::memcpy(h + sizeof(hipIpcMemHandle_t) + sizeof(uint64_t), &p->ipc_nonce, sizeof(uint32_t));
    return PSGD_OK;
}

}  // namespace

extern "C" {

int psgd_ipc_create(psgd_plan* p, int64_t flat_numel, void* handle_out) {
    if (!p || !handle_out) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (p->f64()) return fail(PSGD_ERR_DTYPE, "the IPC all-reduce takes fp32/bf16 plans");
    if (p->wide()) return fail(PSGD_ERR_VALUE, "psgd_ipc_create: ranks above 32 are not supported there");
    if (flat_numel < 0) return fail(PSGD_ERR_VALUE, "negative flat size");
    if (int st = ipc_create_checked(p, flat_numel, handle_out)) return st;
    p->ipc_x2 = false;
    p->ipc_mode = 0;
    return PSGD_OK;
}

int psgd_ipc_create2(psgd_plan* p, int64_t flat_numel, int32_t mode, void* handle_out) {
    if (!p || !handle_out) return fail(PSGD_ERR_VALUE, "null argument");
    if (mode < 0 || mode > 2) return fail(PSGD_ERR_VALUE, "psgd_ipc_create2: mode is 0 (one-shot), 1 (two-shot) or 2 (auto)");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (p->f64()) return fail(PSGD_ERR_DTYPE, "the IPC all-reduce takes fp32/bf16 plans");
    if (!p->wide() && mode == 1)
        return fail(PSGD_ERR_VALUE, "psgd_ipc_create2: the two-shot exchange serves ranks above 32 only");
    if (flat_numel < 0) return fail(PSGD_ERR_VALUE, "negative flat size");
    // the exchange kernels address a slot through 32-bit buffer descriptors and byte offsets
    // (flat_numel first: the sum cannot overflow)
    if (flat_numel >= (int64_t(1) << 30) ||
        (a64(std::max<int64_t>(p->fmax, 1)) + a64(flat_numel)) * int64_t(sizeof(float)) >= (int64_t(1) << 32))
        return fail(PSGD_ERR_VALUE, "psgd_ipc_create2: an exchange slot of 2^32 bytes or more");
    if (int st = ipc_create_checked(p, flat_numel, handle_out)) return st;
    p->ipc_x2 = p->wide();  // a narrow plan's session is psgd_ipc_create's in every respect
    p->ipc_mode = p->wide() ? mode : 0;
    return PSGD_OK;
}

int psgd_ipc_two_shot(const psgd_plan* p, int32_t side, int32_t* out) {
    if (!p || !out) return fail(PSGD_ERR_VALUE, "null argument");
    if (side != 0 && side != 1) return fail(PSGD_ERR_VALUE, "side is 0 (P) or 1 (Q)");
    if (p->ipc_peer.empty()) return fail(PSGD_ERR_STATE, "psgd_ipc_open first");
    *out = p->ipc_two_shot(side) ? 1 : 0;
    return PSGD_OK;
}

int psgd_ipc_shard(int64_t n, int32_t world, int32_t rank, int64_t* begin, int64_t* count) {
    if (!begin || !count) return fail(PSGD_ERR_VALUE, "null argument");
    if (n < 0 || world < 1 || world > kMaxRanks || rank < 0 || rank >= world)
        return fail(PSGD_ERR_VALUE, "bad size/world/rank");
    const int64_t qf = (n + 3) / 4, per = xchg_shard_quads(n, world);
    const int64_t q0 = std::min(per * rank, qf), q1 = std::min(q0 + per, qf);
    *begin = 4 * q0;
    *count = std::max<int64_t>(std::min(4 * q1, n) - 4 * q0, 0);
    return PSGD_OK;
}

int psgd_ipc_open(psgd_plan* p, int32_t world, int32_t rank, const void* handles) {
    if (!p || !handles) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->ipc_buf) return fail(PSGD_ERR_STATE, "psgd_ipc_create first");
    if (!p->ipc_peer.empty()) return fail(PSGD_ERR_STATE, "peers already open (psgd_ipc_close first)");
    if (world < 1 || world > kMaxRanks || rank < 0 || rank >= world) return fail(PSGD_ERR_VALUE, "bad world/rank");
    DevScope scope(p->device);
    const char* hb = static_cast<const char*>(handles);
    std::vector<void*> peer(size_t(world), nullptr);
    std::vector<uint32_t> nonce(size_t(world), 0);
    const XchgChunk own = xchg_arena().chunk(p->ipc_chunk);
    for (int w = 0; w < world; ++w) {
        hipIpcMemHandle_t h;
        uint64_t off = 0;
        const char* e = hb + size_t(w) * kHandleBytes;
        std::memcpy(&h, e, sizeof(h));
        std::memcpy(&off, e + sizeof(h), sizeof(uint64_t));
        std::memcpy(&nonce[w], e + sizeof(h) + sizeof(uint64_t), sizeof(uint32_t));
        if (w == rank) {
            peer[w] = p->ipc_buf;
            if (nonce[w] != p->ipc_nonce || off != uint64_t(p->ipc_off) ||
                std::memcmp(&h, &own.handle, sizeof(h)) != 0)
                return fail(PSGD_ERR_VALUE, "handle list: this rank's entry is not its own exchange handle");
            continue;
        }
        // the peer's chunk, mapped once per process (no unmap / remap between sessions)
        char* base = nullptr;
        if (int st = xchg_arena().map_peer(p->device, h, &base)) return st;
        peer[w] = base + off;
        // the mapping must reach THIS session's region of rank w: its header carries the nonce the
        // handle announced (a stale mapping, or an offset into another session's region, does not)
        uint32_t seen = 0;
        const hipError_t e2 = hipMemcpy(&seen, static_cast<char*>(peer[w]) + kXchgNonceOff, sizeof(uint32_t),
                                        hipMemcpyDeviceToHost);
        if (e2 != hipSuccess || seen != nonce[w])
            return fail(PSGD_ERR_STATE, "the mapping of rank " + std::to_string(w) +
                                            "'s exchange buffer does not reach this session's buffer (stale IPC mapping)");
    }
    p->ipc_peer.assign(peer.begin(), peer.end());
    p->ipc_nonces.assign(nonce.begin(), nonce.end());
    p->ipc_world = world;
    p->ipc_rank = rank;
    return upload_all(p->ws, p->ipc_nonces, p->ipc_peer);
}

int psgd_ipc_close(psgd_plan* p) {
    if (!p) return fail(PSGD_ERR_VALUE, "null plan");
    if (p->ipc_peer.empty()) return PSGD_OK;
    DevScope scope(p->device);
    PSGD_HIP(hipDeviceSynchronize());  // no kernel of this rank still reads a peer buffer
    // the peer mappings stay in the process's arena (mapped once, never unmapped)
    p->ipc_peer.clear();
    p->ipc_world = 0;
    p->ipc_rank = -1;
    if (p->xerr_host) __atomic_store_n(p->xerr_host, 0, __ATOMIC_RELEASE);  // a fresh exchange
    PSGD_HIP(hipMemset(static_cast<char*>(p->ipc_buf) + kXchgErrOff, 0, sizeof(int32_t)));
    return PSGD_OK;
}

int psgd_ipc_debug(psgd_plan* p, int32_t w, psgd_ipc_info* info) {
    if (!p || !info) return fail(PSGD_ERR_VALUE, "null argument");
    std::memset(info, 0, sizeof(*info));
    int64_t c[4];
    xchg_arena().counters(c);
    info->arena_allocs = c[0];
    info->arena_opens = c[1];
    info->arena_reuses = c[2];
    info->arena_frees = c[3];
    info->own_va = uint64_t(reinterpret_cast<uintptr_t>(p->ipc_buf));
    info->own_nonce = p->ipc_nonce;
    if (p->ipc_peer.empty()) return PSGD_OK;
    if (w < 0 || w >= p->ipc_world) return fail(PSGD_ERR_VALUE, "peer out of range");
    DevScope scope(p->device);
    info->peer_va = uint64_t(reinterpret_cast<uintptr_t>(p->ipc_peer[size_t(w)]));
    uint32_t seen = 0;
    PSGD_HIP(hipMemcpy(&seen, static_cast<char*>(p->ipc_peer[size_t(w)]) + kXchgNonceOff, sizeof(uint32_t),
                       hipMemcpyDeviceToHost));
    info->peer_nonce_seen = seen;
    return PSGD_OK;
}

int psgd_ipc_status(psgd_plan* p, int32_t* timed_out) {
    if (!p || !timed_out) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    DevScope scope(p->device);
    PSGD_HIP(hipDeviceSynchronize());  // every enqueued exchange wait has ended
    *timed_out = p->xerr_set() ? 1 : 0;  // sticky until psgd_ipc_close
    return PSGD_OK;
}

int psgd_aggregate_ipc(psgd_plan* p, void* const* grads, void* out, int64_t step, psgd_flat* f, void* const* unc,
                       void* flat_out, void* stream) {
    if (!p || !grads || !out) return fail(PSGD_ERR_VALUE, "null argument");
    if (!p->bound) return fail(PSGD_ERR_STATE, "plan is not bound to device memory");
    if (int st = ipc_check(p, step)) return st;
    if (int st = check_out(out)) return st;
    const bool has_flat = f && f->total > 0;
    if (has_flat) {
        if (int st = check_flat(f, unc && flat_out, f->dtype == PSGD_F32, PSGD_ERR_DTYPE,
                                "psgd_aggregate_ipc packs fp32 uncompressed tensors"))
            return st;
        if (f->total > p->ipc_flat_cap) return fail(PSGD_ERR_VALUE, "flat tensors exceed the exchange buffer (psgd_ipc_create)");
    }
    DevScope scope(p->device);
    return aggregate_ipc_ctx(p, grads, out, step, has_flat ? f : nullptr, unc, flat_out, static_cast<hipStream_t>(stream),
                             nullptr, nullptr);
}

}  // extern "C"
