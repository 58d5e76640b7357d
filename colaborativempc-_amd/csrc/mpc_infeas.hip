// Primal-infeasibility certificate of the structured agent QP (cmpc.h, cmpc_mpc_cert): single-row reachability.
// A hard stage row (k, r) — row_slack[r] == -1, finite h — asks c'x_k <= h with c = C[k, r].  With the adjoint
// recursion
//   p_k = c,  g_j = B_j' p_{j+1},  p_j = A_j' p_{j+1}   (j = k-1 .. 0)
// c'x_k = p_0'x0 + sum_j g_j'u_j, so over the input box its smallest value is
//   reach = p_0'x0 + sum_{j<k, i} min(g_ji lb_i, g_ji ub_i)          (a term with g_ji == 0 counts 0; a term
//                                                                     whose minimising bound is infinite
//                                                                     disqualifies the row)
//   S     = |h| + sum_s |p_0s x0_s| + sum_{j,i} |g_ji| |that bound|   (the scale of the sums' rounding)
// and reach - h > kCertTol S proves the QP infeasible.  The Farkas ray in the layout of cmpc_mpc_duals.y:
//   y_G: 1 at row (k, r); for j < k and input i, t = -g_ji: t on the u_i <= ub_i row when t > 0, -t on the
//        -u_i <= -lb_i row when t < 0; 0 elsewhere
//   y_A: nu_j = -p_j on the state rows j <= k, 0 beyond; 0 on the slack rows and the input-rate rows
// so that G'y_G + A'y_A = 0 and h'y_G + b'y_A = -(reach - h) < 0.
//
// Layout: one wavefront per agent; an agent whose status is 1 or 2 returns at once.  Lanes own candidates
// q = (k-1) nh + (index among the nh hard rows), 64 per pass.  The recursion loop runs j = jtop-1 .. 0 for the
// whole wave, so every lane reads the same A_j, B_j in a step (uniform addresses); a lane joins at j = k-1
// with p = c.  p and the two accumulators stay in registers (static indices only).  Winner: the largest
// (reach - h) / S, ties to the smallest q (k, then r).  A candidate with a non-finite ratio (NaN or infinite
// data) is no candidate: NaN never wins a comparison.  Every element of the ray row is written exactly once.
#include "infeas_ops.h"
#include "internal.h"
#include "wave_ops.h"

namespace cmpc {
namespace {

struct CertPtrs {
    const double* __restrict__ A;
    const double* __restrict__ B;
    const double* __restrict__ x0;
    const double* __restrict__ C;
    const double* __restrict__ h;
    int* status;     // in-out, optional
    double* ray;     // optional
    double* margin;  // optional
    int* row;        // optional
};

__global__ __launch_bounds__(kWave) void mpc_infeas_kernel(const MpcConst c, const CertPtrs P) {
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    if (P.status) {
        const int st = P.status[b];
        if (st == CMPC_SOLVED || st == CMPC_SOLVED_INACCURATE) return;  // (the whole wave: one agent)
    }
    const int nx = c.nx, nu = c.nu, N = c.N, ns = c.ns, mc = c.mc, ms = c.ms, m = c.m, n = c.n;
    const int ne = nx + ns;
    const double* gA = P.A + b * N * nx * nx;
    const double* gB = P.B + b * N * nx * nu;
    const double* gx = P.x0 + b * nx;
    const double* gC = P.C + b * N * mc * nx;
    const double* gh = P.h + b * N * mc;
    const double qnan = __builtin_nan(""), inf = __builtin_inf();

    bool box = true;  // u_lb <= u_ub on every input (a NaN bound passes here and disqualifies its terms below)
    for (int i = 0; i < nu; ++i)
        if (c.u_lb[i] > c.u_ub[i]) box = false;
    int nh = 0;
    for (int r = 0; r < mc; ++r)
        if (c.row_slack[r] < 0) ++nh;
    const int ncand = box ? N * nh : 0;

    double best = -inf;
    int best_q = 0;
    bool best_cert = false;
    for (int q0 = 0; q0 < ncand; q0 += kWave) {
        const int q = q0 + lane;
        const bool in = q < ncand;
        const int qq = in ? q : q0;  // a lane past the end redoes the pass's first candidate and drops it
        const int ks = qq / nh;      // stage k = ks + 1
        const int r = hard_row(c, qq - ks * nh);
        const double hv = gh[ks * mc + r];
        double p[CMPC_MAX_NX], g[CMPC_MAX_NU];
#pragma unroll
        for (int s = 0; s < CMPC_MAX_NX; ++s) p[s] = s < nx ? gC[((size_t)ks * mc + r) * nx + s] : 0.0;
        double reach = 0.0, S = 0.0;
        bool disq = false;
        const int last = q0 + kWave - 1 < ncand ? q0 + kWave - 1 : ncand - 1;
        for (int j = last / nh; j >= 0; --j) {  // (last / nh + 1: the pass's largest stage)
            const bool on = j <= ks;
            adjoint_step(nx, nu, gA + (size_t)j * nx * nx, gB + (size_t)j * nx * nu, p, g, on);
#pragma unroll
            for (int i = 0; i < CMPC_MAX_NU; ++i) {
                if (i < nu) {
                    const double gi = g[i];
                    const double bnd = gi > 0.0 ? c.u_lb[i] : c.u_ub[i];
                    const bool term = on && gi != 0.0;  // (a NaN g is a term: it poisons reach)
                    const bool fin = isfinite(bnd);
                    disq = disq || (term && !fin);
                    reach += (term && fin) ? gi * bnd : 0.0;
                    S += (term && fin) ? fabs(gi) * fabs(bnd) : 0.0;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < CMPC_MAX_NX; ++s) {
            if (s < nx) {
                const double v = p[s] * gx[s];
                reach += v;
                S += fabs(v);
            }
        }
        S += fabs(hv);
        const double d = reach - hv;
        const double ratio = d / S;
        // isfinite(hv): a row with an infinite bound is inactive; isfinite(ratio): NaN falls through
        const bool valid = in && !disq && isfinite(hv) && isfinite(ratio);
        if (valid && ratio > best) {  // (strict: an earlier pass holds the smaller q)
            best = ratio;
            best_q = q;
            best_cert = d > kCertTol * S;
        }
    }

    // ---- winner: the largest ratio, ties to the smallest candidate index ----
    const double top = wave_max(best);
    const bool have = top > -inf;
    const double qmin = wave_min((have && best == top) ? (double)best_q : inf);
    const bool win = have && best == top && (double)best_q == qmin;
    const bool cert = wave_max((win && best_cert) ? 1.0 : 0.0) > 0.0;
    const int qw = have ? __builtin_amdgcn_readfirstlane((int)qmin) : 0;
    const int kw = nh ? qw / nh : 0;  // stage kw + 1
    const int rw = nh ? hard_row(c, qw - kw * nh) : 0;
    const int roww = kw * mc + rw;
    if (lane == 0) {
        if (cert && P.status) P.status[b] = CMPC_PRIMAL_INFEASIBLE;
        if (P.margin) P.margin[b] = have ? top : qnan;
        if (P.row) P.row[b] = cert ? roww : -1;
    }
    if (!P.ray) return;
    const size_t nxa = (size_t)ne * (N + 1), ny = (size_t)m + nxa + n;
    double* y = P.ray + b * ny;
    if (!cert) {
        for (size_t e = lane; e < ny; e += kWave) y[e] = qnan;
        return;
    }
    // ---- the ray: every element once.  First what the recursion does not reach ----
    for (int e = lane; e < ms; e += kWave) y[e] = e == roww ? 1.0 : 0.0;
    for (int e = ms + 2 * nu * (kw + 1) + lane; e < m; e += kWave) y[e] = 0.0;  // input rows of stages j >= k
    for (size_t e = lane; e < nxa; e += kWave) {
        const int j = (int)(e / ne), s = (int)(e - (size_t)j * ne);
        if (s >= nx || j > kw + 1) y[m + e] = 0.0;  // slack rows; state rows beyond stage k
    }
    for (size_t e = lane; e < (size_t)n; e += kWave) y[(size_t)m + nxa + e] = 0.0;  // input-rate rows
    // ... then the winner's recursion again, the same on every lane: lane s stores nu_j[s], lane i the
    // multipliers of input i's two bound rows
    double p[CMPC_MAX_NX], g[CMPC_MAX_NU];
#pragma unroll
    for (int s = 0; s < CMPC_MAX_NX; ++s) p[s] = s < nx ? gC[(size_t)roww * nx + s] : 0.0;
    auto put_nu = [&](int j) {
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < CMPC_MAX_NX; ++s) v = lane == s ? p[s] : v;
        if (lane < nx) y[(size_t)m + (size_t)j * ne + lane] = -v;
    };
    for (int j = kw; j >= 0; --j) {
        put_nu(j + 1);
        adjoint_step(nx, nu, gA + (size_t)j * nx * nx, gB + (size_t)j * nx * nu, p, g, true);
        double gv = 0.0;
#pragma unroll
        for (int i = 0; i < CMPC_MAX_NU; ++i) gv = lane == i ? g[i] : gv;
        if (lane < nu) {
            const double t = -gv;
            const size_t r0 = (size_t)ms + 2 * ((size_t)j * nu + lane);
            y[r0] = t > 0.0 ? t : 0.0;
            y[r0 + 1] = t < 0.0 ? -t : 0.0;
        }
    }
    put_nu(0);
}

}  // namespace

hipError_t mpc_infeas_launch(const MpcConst& c, const MpcPtrs& p, int* status, double* ray, double* margin, int* row,
                             int batch, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    const CertPtrs d{p.A, p.B, p.x0, p.C, p.h, status, ray, margin, row};
    hipLaunchKernelGGL(mpc_infeas_kernel, dim3(batch), dim3(kWave), 0, s, c, d);
    return hipGetLastError();
}

}  // namespace cmpc
