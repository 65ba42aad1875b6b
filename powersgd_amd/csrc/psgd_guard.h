// Skipping a non-finite step on the device (psgd_guard_outputs, include/psgd.h): the argument
// structs and launchers shared by the driver (psgd_guard.cpp) and the kernels (psgd_guard.hip).
//
// Whatever non-finite value enters a compressing step is in data the step has already produced and
// that is small: the gradient enters every product of every iteration, so NaN * x, inf * 0 and
// inf - inf all land in the out-factor the step leaves in the plan's P / Q state, and a non-finite
// uncompressed value is in the dense slab of uncompressed averages. k_guard_check scans those three
// ranges for an all-ones exponent and raises one flag word; k_guard_apply reads the word and, on a
// finite step, returns at once from every workgroup.
#pragma once

#include "psgd_internal.h"

namespace psgd {

constexpr int kGuardCheckWg = 1024;  // at most this many workgroups per scanned range
constexpr int kGuardApplyWg = 1024;  // at most this many workgroups of k_guard_apply (it strides over its units)
constexpr int kGuardUnitVecs = 8;    // 16-byte vectors per thread of one unit of k_guard_apply
constexpr int kGuardUnit = kGuardUnitVecs * kBlock * 16;  // bytes of one unit (a multiple of every element size)

// three dense ranges (0: P state, 1: Q state, 2: the uncompressed slab), each of its own element
// type (psgd_dtype); workgroups [0, nwg[0]) serve range 0, the next nwg[1] range 1, the rest range 2
struct GuardCheckArgs {
    const void* base[3];
    int64_t numel[3];
    int32_t dtype[3];
    int32_t nwg[3];
    unsigned long long* flag;   // one word, never cleared: a finding workgroup raises it to `epoch`
    unsigned long long epoch;   // this call's (every call of a plan takes the next one)
};

// k_guard_apply work item: `bytes` (<= kGuardUnit) of gradient tensor `tensor` from byte `off`
struct GuardItem {
    int64_t off;
    int32_t tensor, bytes;
};

// The units of one k_guard_apply launch, in this order: the gradient items (through the pointer
// table), then kGuardUnit-byte pieces of the two dense ranges it zeroes (0: the compressed output
// slab, 1: the uncompressed slab) and of the two it copies (0: P <- p_init, 1: Q <- q_init)
struct GuardApplyArgs {
    const GuardItem* items;
    void* const* grads;
    int64_t nitems;
    void* zero[2];
    int64_t zbytes[2];
    void* cdst[2];
    const void* csrc[2];
    int64_t cbytes[2];
    int32_t esz, fesz;          // element size of the gradients / outputs, and of the factors
    const unsigned long long* flag;
    unsigned long long epoch;
    long long* result;          // [0]: this call skipped (0 / 1), [1]: += [0]
};

hipError_t launch_guard_check(const GuardCheckArgs& a, hipStream_t s);
hipError_t launch_guard_apply(const GuardApplyArgs& a, hipStream_t s);

}  // namespace psgd
