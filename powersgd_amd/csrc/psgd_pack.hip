// Element-wise copies between tensors and packed buffers: the flat pack of uncompressed
// tensors (k_flat_pack) and the DDP comm hook's bucket passes (k_runs).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "psgd_internal.h"
#include "psgd_stream.cuh"

namespace psgd {

// ---------------------------------------------------------------- flat pack
// reference powersgd.py:22-31 + utils.py:6-10, :43-49: flat = x / W (division, as div_),
// then x = 0. One read + two writes per element.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_flat_pack(FlatArgs a) {
    flat_pack_item<T, kBlock>(a, blockIdx.x);
}

hipError_t launch_flat_pack(int dtype, const FlatArgs& a, hipStream_t s) {
    if (a.nitems == 0) return hipSuccess;
    if (dtype == 2) return launch_flat_pack_f64(a, s);
    if (dtype == 0)
        k_flat_pack<float><<<a.nitems, kBlock, 0, s>>>(a);
    else
        k_flat_pack<bf16_t><<<a.nitems, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- DDP run tables
// The DDP comm hook's two bucket passes (powersgd_amd/ddp.py): ADD folds a bucket
// of fresh gradients into the per-parameter error-feedback residual (what autograd's
// accumulation into p.grad does in the reference flow, README.md:39-42: one add in the
// gradient dtype, bf16 rounded to nearest even), GATHER copies the averaged gradients back into
// the bucket's layout. One item per workgroup: 16 coalesced elements per thread, every load in
// flight before any store.
template <typename T>
struct RunMath {  // fp32 / fp64: native adds
    using A = T;
    static __device__ __forceinline__ A up(T x) { return x; }
    static __device__ __forceinline__ T down(A x) { return x; }
};
template <>
struct RunMath<bf16_t> {
    using A = float;
    static __device__ __forceinline__ A up(bf16_t x) { return bf2f(x); }
    static __device__ __forceinline__ bf16_t down(A x) { return f2bf(x); }
};

template <typename T, bool ADD>
__global__ __launch_bounds__(kBlock) void k_runs(RunsArgs a) {
    using M = RunMath<T>;
    const RunItem it = a.items[blockIdx.x];
    T* t = static_cast<T*>(a.tensors[it.tensor]) + it.toff;
    T* b = static_cast<T*>(a.bucket) + it.boff;
    constexpr int PER = kRunItem / kBlock;
    T v[PER], w[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int j = q * kBlock + int(threadIdx.x);
        const int jj = j < it.cnt ? j : 0;  // clamped, unconditional
        if constexpr (ADD) {
            v[q] = b[jj];
            w[q] = t[jj];
        } else {
            v[q] = t[jj];
        }
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int j = q * kBlock + int(threadIdx.x);
        if (j < it.cnt) {
            if constexpr (ADD)
                t[j] = M::down(M::up(w[q]) + M::up(v[q]));  // residual + fresh gradient
            else
                b[j] = v[q];
        }
    }
}

template <typename T>
hipError_t launch_runs_t(bool add, const RunsArgs& a, hipStream_t s) {
    if (add)
        k_runs<T, true><<<a.nitems, kBlock, 0, s>>>(a);
    else
        k_runs<T, false><<<a.nitems, kBlock, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_runs(int dtype, bool add, const RunsArgs& a, hipStream_t s) {
    if (a.nitems <= 0) return hipSuccess;
    if (dtype == 0) return launch_runs_t<float>(add, a, s);
    if (dtype == 2) return launch_runs_t<double>(add, a, s);
    return launch_runs_t<bf16_t>(add, a, s);
}

// ---------------------------------------------------------------- mixed / source-table runs
// psgd_runs_create_mixed's tables beyond k_runs: bucket side in B, tensor side in T (the pair
// (bf16, fp32): an fp32 error-feedback residual fed by bf16 gradients), the bucket side either one
// buffer or, with LIST, a table of source tensors (item i reads sources[src[i]]).
//   ADD     tensor = tensor + up(bucket): for (bf16, fp32) an exact upcast and ONE fp32 add, no
//           rounding to bf16 anywhere; equal pairs as k_runs. kRunsAddZero also stores +0.0 to the
//           bucket side (the consumed gradients, zeroed in the pass that reads them).
//   GATHER  bucket = down(tensor): for (bf16, fp32) round to nearest even (f2bf).
// Same item shape as k_runs: up to kRunItem elements of one run, 64-bit element offsets, loads
// unconditional from clamped addresses and all issued before the first store. The two sides are
// aligned independently (2 bytes / 4 bytes for the mixed pair): one element per lane access.
template <typename B, typename T>
struct RunConv {  // equal pairs: the tensors' own arithmetic
    using A = typename RunMath<T>::A;
    static __device__ __forceinline__ A up_b(B x) { return RunMath<T>::up(x); }
    static __device__ __forceinline__ B down_b(T x) { return x; }
};
template <>
struct RunConv<bf16_t, float> {
    using A = float;
    static __device__ __forceinline__ A up_b(bf16_t x) { return bf2f(x); }
    static __device__ __forceinline__ bf16_t down_b(float x) { return f2bf(x); }
};

template <typename B, typename T, int MODE, bool LIST>
__global__ __launch_bounds__(kBlock) void k_runs_mix(RunsMixArgs a) {
    using C = RunConv<B, T>;
    using M = RunMath<T>;
    constexpr bool ADD = MODE != kRunsGather;
    const RunItem it = a.items[blockIdx.x];
    const gptr<T> t = gmut<T>(a.tensors[it.tensor]) + it.toff;
    void* base = a.bucket;
    if constexpr (LIST) base = a.sources[a.src[blockIdx.x]];
    const gptr<B> b = gmut<B>(base) + it.boff;
    constexpr int PER = kRunItem / kBlock;
    B v[PER];
    T w[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int j = q * kBlock + int(threadIdx.x);
        const int jj = j < it.cnt ? j : 0;  // clamped, unconditional
        if constexpr (ADD) v[q] = b[jj];
        w[q] = t[jj];
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int j = q * kBlock + int(threadIdx.x);
        if (j < it.cnt) {
            if constexpr (ADD) {
                t[j] = M::down(M::up(w[q]) + C::up_b(v[q]));  // residual + fresh gradient
                if constexpr (MODE == kRunsAddZero) b[j] = B(0);
            } else {
                b[j] = C::down_b(w[q]);
            }
        }
    }
}

template <typename B, typename T, bool LIST>
hipError_t launch_runs_mix_t(int mode, const RunsMixArgs& a, hipStream_t s) {
    if (mode == kRunsGather)
        k_runs_mix<B, T, kRunsGather, LIST><<<a.nitems, kBlock, 0, s>>>(a);
    else if (mode == kRunsAdd)
        k_runs_mix<B, T, kRunsAdd, LIST><<<a.nitems, kBlock, 0, s>>>(a);
    else if constexpr (LIST)  // zeroing the bucket side exists in the source-table form only
        k_runs_mix<B, T, kRunsAddZero, true><<<a.nitems, kBlock, 0, s>>>(a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename B, typename T>
hipError_t launch_runs_mix_bt(int mode, const RunsMixArgs& a, hipStream_t s) {
    if (a.src) return launch_runs_mix_t<B, T, true>(mode, a, s);
    if constexpr (std::is_same_v<B, T>)
        return hipErrorInvalidValue;  // equal pair, one bucket: k_runs (launch_runs)
    else
        return launch_runs_mix_t<B, T, false>(mode, a, s);
}

hipError_t launch_runs_mix(int bucket_dtype, int tensor_dtype, int mode, const RunsMixArgs& a, hipStream_t s) {
    if (a.nitems <= 0) return hipSuccess;
    if (bucket_dtype == 1 && tensor_dtype == 0) return launch_runs_mix_bt<bf16_t, float>(mode, a, s);
    if (bucket_dtype != tensor_dtype) return hipErrorInvalidValue;
    if (tensor_dtype == 0) return launch_runs_mix_bt<float, float>(mode, a, s);
    if (tensor_dtype == 2) return launch_runs_mix_bt<double, double>(mode, a, s);
    return launch_runs_mix_bt<bf16_t, bf16_t>(mode, a, s);
}

}  // namespace psgd
