// An inner round's publication of a consensus step (include/cmpc.h, cmpc_lin_publish_dev and cmpc_lpv_publish_dev):
// the one statement of the rule, which lin_publish_kernel (lin_build.hip) and lpv_publish_kernel (lpv_round.hip)
// both run, so the two families cannot drift apart.
#pragma once
#include "internal.h"
#include "wave_ops.h"

namespace cmpc {

// One agent, one wavefront (every lane active): out <- the predicted positions (zb[k nxe + ix], zb[k nxe + iy]),
// k = 0..N, and the allclose test of them against `prev`, the agent's row of the exchange buffer; an agent with a
// non-finite value anywhere in its nz entries publishes `prev` again and is never close.  One lane per position
// entry; the verdict and the largest move go through the wave (nmax keeps a NaN, as numpy's max does), and lane 0
// writes them (close, delta: this agent's entries, may be null) and counts the agent into *not_close (may be null).
// PD = 3 (cmpc_lin3_publish_dev): the positions are (zb[k nxe + ix], zb[k nxe + iy], zb[k nxe + iz]) and `per` is
// 3(N+1); the planar instantiation never reads iz.
template <int PD = 2>
__device__ __forceinline__ void publish_agent(const double* __restrict__ zb, size_t nz, int nxe, int ix, int iy, int per,
                                              const double* __restrict__ prev, double* __restrict__ out, double atol,
                                              double rtol, int* close, double* delta, int* not_close, int iz = 0) {
#pragma clang fp contract(off)
    static_assert(PD == 2 || PD == 3, "positions are planar or 3-D");
    bool bad = false;
    for (size_t i = threadIdx.x; i < nz; i += kWave) bad |= !isfinite(zb[i]);
    bad = __any(bad);  // (the workgroup is one wavefront)
    bool far = bad;
    double dm = 0.0;
    for (int i = threadIdx.x; i < per; i += kWave) {
        const double p = prev[i];
        double v;
        if constexpr (PD == 2) {
            v = bad ? p : zb[(size_t)(i >> 1) * nxe + ((i & 1) ? iy : ix)];
        } else {
            const int k = i / 3, a = i - 3 * k;
            v = bad ? p : zb[(size_t)k * nxe + (a == 0 ? ix : a == 1 ? iy : iz)];
        }
        out[i] = v;
        const double d = fabs(p - v), lim = atol + rtol * fabs(v);
        far |= !(d <= lim);  // NaN is never close (numpy equal_nan=False)
        dm = nmax(d, dm);
    }
    far = __any(far);
    dm = wave_max(dm);  // (every lane is active here)
    if (threadIdx.x == 0) {
        if (close) *close = far ? 0 : 1;
        if (delta) *delta = bad ? __builtin_nan("") : dm;
        if (not_close && far) atomicAdd(not_close, 1);
    }
}

}  // namespace cmpc
