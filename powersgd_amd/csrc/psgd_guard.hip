// Kernels of psgd_guard_outputs (psgd_guard.h): k_guard_check scans the plan's P / Q state and the
// dense uncompressed slab for a non-finite value and raises one flag word; k_guard_apply reads the
// word and, when the step is to be skipped, zeroes the gradients, the outputs and the uncompressed
// slab and copies the retained initial factors over P and Q. On a finite step every workgroup of
// k_guard_apply returns at once and writes nothing (workgroup 0 writes result[0] = 0).
//
// Codegen rules as everywhere in the codec: global pointers in address space
// 1, unconditional loads from clamped addresses masked by selects, no float atomics, no scratch.
// The verdict is one bit, so the integer atomic max that raises the word is order-independent.
#include <hip/hip_runtime.h>

#include "psgd_guard.h"
#include "psgd_stream.cuh"

namespace psgd {

namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// Non-finite = an all-ones exponent field, tested on the bits (a floating-point comparison such as
// x - x != 0 may be folded away under the build's arithmetic flags). `vec`: one 16-byte vector of
// V elements at a 16-byte boundary; `one`: the raw bits of a single element.
template <typename T>
struct GuardIo;
template <>
struct GuardIo<float> {
    static constexpr int V = 4;
    typedef uint32_t bits;
    static __device__ __forceinline__ bool one(bits x) { return (x & 0x7f800000u) == 0x7f800000u; }
    static __device__ __forceinline__ bool vec(const v4u& x) {
        bool b = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) b |= one(x[e]);
        return b;
    }
};
template <>
struct GuardIo<bf16_t> {
    static constexpr int V = 8;
    typedef uint16_t bits;
    static __device__ __forceinline__ bool one(bits x) { return (x & 0x7f80u) == 0x7f80u; }
    static __device__ __forceinline__ bool vec(const v4u& x) {
        bool b = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) b |= ((x[e] & 0x7f80u) == 0x7f80u) | ((x[e] & 0x7f800000u) == 0x7f800000u);
        return b;
    }
};
template <>
struct GuardIo<double> {
    static constexpr int V = 2;
    typedef unsigned long long bits;
    static __device__ __forceinline__ bool one(bits x) { return ((x >> 52) & 0x7ffull) == 0x7ffull; }
    // little endian: words 1 and 3 hold the two elements' sign, exponent and high mantissa
    static __device__ __forceinline__ bool vec(const v4u& x) {
        return ((x[1] & 0x7ff00000u) == 0x7ff00000u) | ((x[3] & 0x7ff00000u) == 0x7ff00000u);
    }
};

// Workgroup `w` of the `nwg` of one range of n elements at p, split as k_norm_stream splits its
// ranges: [head | 16-byte vectors | tail], the head up to the first 16-byte boundary (fewer than V
// elements), the tail what no whole vector covers; workgroup 0 also takes head and tail, one
// element per thread. Returns whether this thread saw a non-finite element.
template <typename T>
__device__ __forceinline__ bool guard_scan(const void* base, int64_t n, int w, int nwg) {
    using Io = GuardIo<T>;
    typedef typename Io::bits bits;
    constexpr int V = Io::V;
    const bits* p = static_cast<const bits*>(base);
    const int64_t mis = int64_t((reinterpret_cast<uintptr_t>(p) & 15) / sizeof(bits));
    int64_t head = mis ? V - mis : 0;
    if (head > n) head = n;
    const int64_t nvec = (n - head) / V, tail = n - head - nvec * V;
    const int64_t per = (nvec + nwg - 1) / nwg;
    const int64_t lo = int64_t(w) * per, hi = lo + per < nvec ? lo + per : nvec;
    const gptr<const v4u> body = (gptr<const v4u>)(reinterpret_cast<const v4u*>(p + head));
    bool bad = false;
    for (int64_t b = lo; b < hi; b += 4 * kBlock) {
        v4u x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = b + u * kBlock + threadIdx.x;
            x[u] = body[i < hi ? i : hi - 1];  // clamped, unconditional (a re-read of an in-range vector)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) bad |= Io::vec(x[u]);
    }
    if (w == 0) {  // head and tail: fewer than 2 V elements
        const int64_t ns = head + tail, t = threadIdx.x;
        const int64_t i = t < head ? t : n - tail + (t - head);
        const bits x = gconst<bits>(p)[t < ns ? i : 0];
        bad |= t < ns ? Io::one(x) : false;
    }
    return bad;
}

// `bytes` zero bytes at p for the workgroup (bytes <= kGuardUnit, p aligned to esz, bytes a multiple
// of esz): a head up to the first 16-byte boundary and a tail in element-sized stores, one per
// thread, 16-byte vector stores between. Nothing outside [p, p + bytes) is touched.
__device__ __forceinline__ void guard_zero(char* p, int bytes, int esz) {
    const int mis = int(reinterpret_cast<uintptr_t>(p) & 15);
    int head = mis ? 16 - mis : 0;
    if (head > bytes) head = bytes;
    const int nvec = (bytes - head) >> 4, tail = bytes - head - 16 * nvec;
    const int tid = int(threadIdx.x);
    const gptr<v4u> body = (gptr<v4u>)(reinterpret_cast<v4u*>(p + head));
    const v4u z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < kGuardUnitVecs; ++q) {
        const int i = q * kBlock + tid;
        if (i < nvec) body[i] = z;
    }
    const int o = tid * esz;  // head and tail: at most 30 bytes, one element per thread
    if (o < head + tail) {
        char* e = p + (o < head ? o : bytes - tail + (o - head));
        if (esz == 2)
            *(gptr<uint16_t>)(reinterpret_cast<uint16_t*>(e)) = uint16_t(0);
        else if (esz == 4)
            *(gptr<uint32_t>)(reinterpret_cast<uint32_t*>(e)) = 0u;
        else
            *(gptr<unsigned long long>)(reinterpret_cast<unsigned long long*>(e)) = 0ull;
    }
}

// `bytes` bytes from src to dst, element by element (fesz 4 or 8: the two bases share no alignment
// beyond their element's); the bits are copied as integers
__device__ __forceinline__ void guard_copy(char* dst, const char* src, int bytes, int fesz) {
    if (fesz == 4) {
        const gptr<const uint32_t> s = gconst<uint32_t>(src);
        const gptr<uint32_t> d = gmut<uint32_t>(dst);
        for (int i = int(threadIdx.x); i < (bytes >> 2); i += kBlock) d[i] = s[i];
    } else {
        const gptr<const unsigned long long> s = gconst<unsigned long long>(src);
        const gptr<unsigned long long> d = gmut<unsigned long long>(dst);
        for (int i = int(threadIdx.x); i < (bytes >> 3); i += kBlock) d[i] = s[i];
    }
}

__device__ __forceinline__ int64_t guard_pieces(int64_t bytes) { return (bytes + kGuardUnit - 1) / kGuardUnit; }

}  // namespace

__global__ __launch_bounds__(kBlock) void k_guard_check(GuardCheckArgs a) {
    const int blk = int(blockIdx.x);
    const int which = blk < a.nwg[0] ? 0 : blk < a.nwg[0] + a.nwg[1] ? 1 : 2;
    const int w = blk - (which > 0 ? a.nwg[0] : 0) - (which > 1 ? a.nwg[1] : 0);
    const int dtype = a.dtype[which];  // workgroup-uniform
    bool bad;
    if (dtype == 0)
        bad = guard_scan<float>(a.base[which], a.numel[which], w, a.nwg[which]);
    else if (dtype == 1)
        bad = guard_scan<bf16_t>(a.base[which], a.numel[which], w, a.nwg[which]);
    else
        bad = guard_scan<double>(a.base[which], a.numel[which], w, a.nwg[which]);
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (any && threadIdx.x == 0) __hip_atomic_fetch_max(a.flag, a.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void k_guard_apply(GuardApplyArgs a) {
    const unsigned long long word =
        __hip_atomic_load(const_cast<unsigned long long*>(a.flag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool skip = word == a.epoch;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const gptr<long long> res = gmut<long long>(a.result);
        res[0] = skip ? 1 : 0;
        if (skip) res[1] = res[1] + 1;
    }
    if (!skip) return;
    const int64_t nz0 = guard_pieces(a.zbytes[0]), nz1 = guard_pieces(a.zbytes[1]);
    const int64_t nc0 = guard_pieces(a.cbytes[0]), nc1 = guard_pieces(a.cbytes[1]);
    const int64_t total = a.nitems + nz0 + nz1 + nc0 + nc1;
    for (int64_t u = blockIdx.x; u < total; u += gridDim.x) {
        if (u < a.nitems) {
            const GuardItem it = a.items[u];
            guard_zero(static_cast<char*>(a.grads[it.tensor]) + it.off, it.bytes, a.esz);
            continue;
        }
        int64_t k = u - a.nitems;
        if (k < nz0 + nz1) {
            const int r = k < nz0 ? 0 : 1;
            k -= r ? nz0 : 0;
            const int64_t o = k * kGuardUnit, left = a.zbytes[r] - o;
            guard_zero(static_cast<char*>(a.zero[r]) + o, int(left < kGuardUnit ? left : kGuardUnit), a.esz);
            continue;
        }
        k -= nz0 + nz1;
        const int r = k < nc0 ? 0 : 1;
        k -= r ? nc0 : 0;
        const int64_t o = k * kGuardUnit, left = a.cbytes[r] - o;
        guard_copy(static_cast<char*>(a.cdst[r]) + o, static_cast<const char*>(a.csrc[r]) + o,
                   int(left < kGuardUnit ? left : kGuardUnit), a.fesz);
    }
}

hipError_t launch_guard_check(const GuardCheckArgs& a, hipStream_t s) {
    const int n = a.nwg[0] + a.nwg[1] + a.nwg[2];
    if (n == 0) return hipSuccess;
    k_guard_check<<<n, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_guard_apply(const GuardApplyArgs& a, hipStream_t s) {
    auto pieces = [](int64_t bytes) { return (bytes + kGuardUnit - 1) / kGuardUnit; };
    const int64_t total = a.nitems + pieces(a.zbytes[0]) + pieces(a.zbytes[1]) + pieces(a.cbytes[0]) + pieces(a.cbytes[1]);
    const int n = int(std::max<int64_t>(1, std::min<int64_t>(kGuardApplyWg, total)));  // one at least: result[0]
    k_guard_apply<<<n, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace psgd
