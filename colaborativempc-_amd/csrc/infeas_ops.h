// The adjoint recursion of the infeasibility certificates (mpc_infeas.hip, mpc_infeas_rows.hip): one lane, one row.
#pragma once
#include "internal.h"

namespace cmpc {

// g = B_j' p, then p <- A_j' p where `on`
__device__ __forceinline__ void adjoint_step(int nx, int nu, const double* __restrict__ Aj,
                                             const double* __restrict__ Bj, double (&p)[CMPC_MAX_NX],
                                             double (&g)[CMPC_MAX_NU], bool on) {
    double pn[CMPC_MAX_NX];
#pragma unroll
    for (int t = 0; t < CMPC_MAX_NX; ++t) pn[t] = 0.0;
#pragma unroll
    for (int i = 0; i < CMPC_MAX_NU; ++i) g[i] = 0.0;
#pragma unroll
    for (int s = 0; s < CMPC_MAX_NX; ++s) {
        if (s < nx) {
            const double ps = p[s];
#pragma unroll
            for (int i = 0; i < CMPC_MAX_NU; ++i)
                if (i < nu) g[i] = fma(Bj[s * nu + i], ps, g[i]);
#pragma unroll
            for (int t = 0; t < CMPC_MAX_NX; ++t)
                if (t < nx) pn[t] = fma(Aj[s * nx + t], ps, pn[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < CMPC_MAX_NX; ++t) p[t] = on ? pn[t] : p[t];
}

// the r of the jr-th hard row (row_slack < 0)
__device__ __forceinline__ int hard_row(const MpcConst& c, int jr) {
    int r = 0, cnt = 0;
    for (int rr = 0; rr < c.mc; ++rr) {
        if (c.row_slack[rr] < 0) {
            r = cnt == jr ? rr : r;
            ++cnt;
        }
    }
    return r;
}

}  // namespace cmpc
