// Orthonormalisation of the in-factor: the one translation unit of every orthonormalisation
// kernel. The Householder kernels (psgd_orth_householder.cuh) and the Cholesky-QR kernels
// (psgd_orth_chol.cuh) share the out-of-line householder_q instances of psgd_chain.cuh, so
// they are compiled together.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "psgd_internal.h"
#include "psgd_orth_householder.cuh"
#include "psgd_orth_chol.cuh"

namespace psgd {

hipError_t launch_orth_chain(const ChainArgs& a, int nunits, int64_t max_rows, int R, hipStream_t s) {
    if (nunits == 0) return hipSuccess;
    auto grid = [&](int nt) { return dim3(unsigned(nunits), unsigned((max_rows + PSGD_CHAIN_ROWS * nt - 1) / (PSGD_CHAIN_ROWS * nt))); };
    switch (R) {
        case 2: k_orth_chain<2><<<grid(PSGD_CHAIN_NT), PSGD_CHAIN_NT, 0, s>>>(a); break;
        case 4: k_orth_chain<4><<<grid(PSGD_CHAIN_NT), PSGD_CHAIN_NT, 0, s>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_orth_mgs(const OrthArgs& a, int nunits, int R, hipStream_t s) {
    switch (R) {
        case 1: k_orth_mgs<1><<<nunits, kBlock, 0, s>>>(a); break;
        case 2: k_orth_mgs<2><<<nunits, kBlock, 0, s>>>(a); break;
        case 4: k_orth_mgs<4><<<nunits, kBlock, 0, s>>>(a); break;
        case 8: k_orth_mgs<8><<<nunits, kBlock, 0, s>>>(a); break;
        case 16: k_orth_mgs<16><<<nunits, kBlock, 0, s>>>(a); break;
        case 32: k_orth_mgs<32><<<nunits, kBlock, 0, s>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_orth(const OrthArgs& a, int nunits, int R, int64_t kmax, bool chol, hipStream_t s) {
    if (R == 1) return launch_orth_reg<1>(1, a, nunits, s);  // the joint norm of every group
    static const int diag = [] {
        const char* e = std::getenv("PSGD_ORTH_DIAG");
        return e ? std::atoi(e) : 0;
    }();
    if (chol && R <= 32) {
        OrthArgs b = a;
        b.flags = diag;
        return launch_orth_chol(b, nunits, R, kmax, s);
    }
    const OrthChoice c = orth_select(R, kmax);
    switch (c.kernel) {
        case OrthKernel::Wy:
            return R == 2 ? launch_orth_wy<2>(c.rpt, c.nw, a, nunits, s)
                 : R == 4 ? launch_orth_wy<4>(c.rpt, c.nw, a, nunits, s)
                 : R == 8 ? launch_orth_wy<8>(c.rpt, c.nw, a, nunits, s) : hipErrorInvalidValue;
        case OrthKernel::Reg:
            return R == 2 ? launch_orth_reg<2>(c.rpt, a, nunits, s)
                 : R == 4 ? launch_orth_reg<4>(c.rpt, a, nunits, s)
                 : R == 8 ? launch_orth_reg<8>(c.rpt, a, nunits, s) : hipErrorInvalidValue;
        case OrthKernel::Lds: return launch_orth_lds(R, a, nunits, c.lds_floats, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace psgd
