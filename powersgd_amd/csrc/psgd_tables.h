// Word tables of the update entries (psgd_sgd.cpp, psgd_adam.cpp): a TableCache over 8-byte words
// with a device allocation that grows on demand, and the helpers that lay pointers, work items and
// hyperparameter records out as words.
#pragma once
#include <cstring>
#include <vector>

#include "psgd_plan.h"

namespace psgd {

struct WordTable {
    psgd::TableCache t;
    char* dev = nullptr;
    size_t cap = 0;
    // a table of `words` entries: bind, grow or re-bind; launches on `s` may still read the old one
    int room(size_t words, hipStream_t s) {
        if (dev && words <= cap && t.n == words) return PSGD_OK;
        if (dev) PSGD_HIP(hipStreamSynchronize(s));
        if (!dev || words > cap) {
            release();
            PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&dev), psgd::TableCache::bytes(words)));
            cap = words;
        }
        t.bind(dev, words);
        return PSGD_OK;
    }
    // the words' device copy (selected, or uploaded stream-ordered)
    int select(const std::vector<void*>& words, hipStream_t s, const void** out) {
        if (int st = room(words.size(), s)) return st;
        PSGD_HIP(t.select(words.data(), s));
        *out = t.table();
        return PSGD_OK;
    }
    void release() {
        t.release();
        if (dev) (void)hipFree(dev);
        dev = nullptr;
        cap = 0;
    }
    ~WordTable() { release(); }
};

// The ADD of the flat plan's tensors in the master-weight entries (residual += float(g); g = +0.0):
// a run table over that plan's element counts with its workspace, made at the first call and again
// when the counts change
struct FlatAdd {
    psgd_runs* runs = nullptr;
    char* ws = nullptr;
    std::vector<int64_t> numel;
    void drop() {
        if (runs) (void)psgd_runs_destroy(runs);
        if (ws) (void)hipFree(ws);
        runs = nullptr;
        ws = nullptr;
    }
    int add(int device, const psgd_flat* f, void* const* unc16, void* const* unc_residual, hipStream_t s) {
        const size_t nu = size_t(f->count);
        std::vector<int64_t> want(nu, 0);
        for (const FlatEntry& en : f->entries) want[size_t(en.tensor)] = en.numel;
        if (!runs || numel != want) {
            if (runs) PSGD_HIP(hipStreamSynchronize(s));
            drop();
            std::vector<int64_t> zero(nu, 0);
            std::vector<int32_t> idx(nu);
            for (size_t i = 0; i < nu; ++i) idx[i] = int32_t(i);
            if (int st = psgd_runs_create_mixed(zero.data(), idx.data(), zero.data(), want.data(), idx.data(), int32_t(nu),
                                                int32_t(nu), int32_t(nu), PSGD_BF16, PSGD_F32, &runs))
                return st;
            int64_t rb = 0;
            if (int st = psgd_runs_workspace_bytes(runs, &rb)) return st;
            PSGD_HIP(hipMalloc(reinterpret_cast<void**>(&ws), size_t(rb > 1 ? rb : 1)));
            if (int st = psgd_runs_bind(runs, device, ws)) return st;
            numel = want;
        }
        return psgd_runs_add_list(runs, unc16, unc_residual, 1, s);
    }
    ~FlatAdd() { drop(); }
};

inline void put(std::vector<void*>& w, const void* src, size_t bytes) {
    const size_t at = w.size();
    w.resize(at + (bytes + sizeof(void*) - 1) / sizeof(void*), nullptr);
    if (bytes) std::memcpy(w.data() + at, src, bytes);
}

inline void put_ptrs(std::vector<void*>& w, void* const* ptrs, size_t n) {
    if (ptrs) w.insert(w.end(), ptrs, ptrs + n);
    else w.resize(w.size() + n, nullptr);
}

}  // namespace psgd
