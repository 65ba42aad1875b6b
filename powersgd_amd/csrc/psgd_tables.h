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
