// Self test of the fused row-broadcast fma (wave_ops.h), reached through cmpc_selftest_fma_bcast.
#include "internal.h"
#include "wave_ops.h"

namespace cmpc {

// Every lane J, both signs, both forms, against the two-instruction expression on the same inputs.
// The broadcast source is recomputed per case, x' = fma(x, 1, -0) (x to the bit; the factors come
// from memory, one pair per case, so it is neither folded nor shared), and the scheduling barriers
// keep that fma in front of the fused form, inside the two wait states the nop has to supply (at
// most the copy of the addend into the tied destination between them): the read-after-write case
// as the kernel's chains build it.  Cases: 0 fma_bcast16, 1 fnma_bcast16, 2 fma_bcast16s,
// 3 fnma_bcast16s with the source as its own addend (the panel step's shape).
__global__ void fma_bcast_selftest_kernel(const double* A, const double* X, const double* C, const double* one,
                                          const double* nzero, double* fused, double* ref) {
    const int l = threadIdx.x;
    const double a = A[l], x = X[l], c = C[l];
    static_for<0, 16>([&](auto jc) __attribute__((always_inline)) {
        constexpr int J = decltype(jc)::value;
        double r0, r1, r2, r3;
        {
            __builtin_amdgcn_sched_barrier(0);
            const double xj = fma(x, one[4 * J], nzero[4 * J]);
            r0 = fma_bcast16<J>(a, xj, c);
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            const double xj = fma(x, one[4 * J + 1], nzero[4 * J + 1]);
            r1 = fnma_bcast16<J>(a, xj, c);
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            const double xj = fma(x, one[4 * J + 2], nzero[4 * J + 2]);
            r2 = fma_bcast16s<J>(a, dpp_settled(xj), c);
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            const double xj = fma(x, one[4 * J + 3], nzero[4 * J + 3]);
            const double xs = dpp_settled(xj);
            r3 = fnma_bcast16s<J>(a, xs, xs);
            __builtin_amdgcn_sched_barrier(0);
        }
        fused[(0 * 16 + J) * 64 + l] = r0;
        fused[(1 * 16 + J) * 64 + l] = r1;
        fused[(2 * 16 + J) * 64 + l] = r2;
        fused[(3 * 16 + J) * 64 + l] = r3;
        const double xb = bcast16<J>(x);
        ref[(0 * 16 + J) * 64 + l] = fma(a, xb, c);
        ref[(1 * 16 + J) * 64 + l] = fma(-xb, a, c);
        ref[(2 * 16 + J) * 64 + l] = fma(a, xb, c);
        ref[(3 * 16 + J) * 64 + l] = fma(-xb, a, x);
    });
}

hipError_t selftest_fma_bcast_launch(const double* A, const double* X, const double* C, const double* one,
                                     const double* nzero, double* fused, double* ref, hipStream_t s) {
    hipLaunchKernelGGL(fma_bcast_selftest_kernel, dim3(1), dim3(kWave), 0, s, A, X, C, one, nzero, fused, ref);
    return hipGetLastError();
}

}  // namespace cmpc
