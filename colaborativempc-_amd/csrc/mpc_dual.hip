// Dual solution of the structured agent QP in OSQP's form (cmpc.h, cmpc_mpc_duals): from the primal
// point z and the inequality multipliers lambda (G's row order) one launch writes, per agent,
//   y = [y_G (m) | y_A (ne (N + 1) + nu N)]   and   dua_res = ||P z + q + G'y_G + A'y_A||_inf.
//   y_G[r]   = lambda[r] where the row's bound is finite, else exactly 0 (a select: the slot may hold anything)
//   nu_d,0   = 2 dR du_0,  nu_d,i = -2 dR du_i (i >= 1)                       (the input-rate rows)
//   g_k      = 2 Q x_k + 2 qlin_k + C_k' lambda_k (the last term for k >= 1)
//   nu_N     = -g_N,  nu_k = A_k' nu_{k+1} - g_k  (k = N-1 .. 0)               (the state rows: costates)
//   0 on the slack rows of A (the empty 0 = 0 rows)
// With these the x and du columns of the stationarity vector vanish up to rounding; the u and slack
// columns carry the dual residual.  An agent whose validity marker is not 1 (a solver exit that holds no
// multipliers of the iterate it returned) or whose z is not finite gets an all-NaN y row and a NaN dua_res.
//
// Layout: 16 lanes (one DPP row) per agent, four agents per wavefront.  Lane t < nx carries nu[t], lanes
// nx .. nx + nu - 1 the u columns of the same stage: one transposed mat-vec [A_k B_k]' nu_{k+1} per stage
// over row broadcasts of nu, every coefficient read with consecutive lanes on consecutive addresses.  The
// chain over the horizon is serial; everything a stage needs besides nu_{k+1} (the coefficients, g_k, the
// u column's own terms) is formed one stage ahead of the chain.  No LDS, no per-agent scratch.
#include "internal.h"
#include "wave_ops.h"

namespace cmpc {
namespace {

constexpr int kRow = 16;           // lanes per agent
constexpr int kDualThreads = 64;   // one wavefront: four agents

struct DualPtrs {
    const double* A;
    const double* B;
    const double* p;
    const double* C;
    const double* h;
    const double* z;
    const double* lam;             // agent b's m multipliers at lam + b * lam_stride
    const double* valid;           // optional: agent b's marker at valid + b * valid_stride (1.0: lam holds z's)
    unsigned long long lam_stride, valid_stride;
    double* y;
    double* dua_res;               // optional
};

__global__ __launch_bounds__(kDualThreads) void mpc_dual_kernel(const MpcConst c, const DualPtrs P, int batch) {
    const int tid = threadIdx.x, t = tid & (kRow - 1);
    const int ag = blockIdx.x * (kDualThreads / kRow) + (tid >> 4);
    const bool live = ag < batch;
    // a row past the batch redoes the last agent and stores nothing: the row broadcasts below want the
    // whole wavefront active
    const size_t b = live ? ag : batch - 1;
    const int nx = c.nx, nu = c.nu, N = c.N, ns = c.ns, mc = c.mc, ms = c.ms, m = c.m, n = c.n;
    const int ne = nx + ns;
    const size_t nz = (size_t)ne * (N + 1) + 2 * (size_t)n, ny = (size_t)m + (size_t)ne * (N + 1) + n;
    const double* gA = P.A + b * N * nx * nx;
    const double* gB = P.B + b * N * nx * nu;
    const double* gp = P.p + b * (N + 1) * nx;
    const double* gC = P.C + b * N * mc * nx;
    const double* gh = P.h + b * N * mc;
    const double* z = P.z + b * nz;
    const double* lam = P.lam + b * P.lam_stride;
    double* y = P.y + b * ny;
    const double* zu = z + (size_t)ne * (N + 1);
    const double* zd = zu + n;
    const double qnan = __builtin_nan("");

    // ---- validity: the marker, and a finite z ----
    double bad = (P.valid && P.valid[b * P.valid_stride] != 1.0) ? 1.0 : 0.0;
    for (size_t i = t; i < nz; i += kRow)
        if (!isfinite(z[i])) bad = 1.0;
    const bool ok = row_reduce(bad, nmax_) == 0.0;
    auto put = [&](size_t i, double v) {
        if (live) y[i] = ok ? v : qnan;
    };

    // multiplier of inequality row r: the solver's where the bound is finite, else exactly 0
    auto yg = [&](int r) -> double {
        double w;
        if (r < ms) {
            w = gh[r];
        } else {
            const int q = r - ms, i = (q >> 1) % nu;
            w = (q & 1) ? -c.u_lb[i] : c.u_ub[i];
        }
        const double lr = lam[r];
        return isfinite(w) ? lr : 0.0;
    };
    // (dR du_i)[j], (R u_k)[j]
    auto drdu = [&](int i, int j) -> double {
        double v = 0.0;
        for (int e = 0; e < nu; ++e) v = fma(c.dR[j * nu + e], zd[i * nu + e], v);
        return v;
    };

    double res = 0.0;
    // ---- y_G, the input-rate rows, the slack rows and the slack columns' residual: independent items ----
    for (int r = t; r < m; r += kRow) put(r, yg(r));
    for (int e = t; e < n; e += kRow) {
        const int i = e / nu, j = e - i * nu;
        const double v = 2.0 * drdu(i, j);
        put((size_t)m + (size_t)ne * (N + 1) + e, i ? -v : v);
    }
    for (int e = t; e < (N + 1) * ns; e += kRow) {
        const int k = e / ns, j = e - k * ns;
        put((size_t)m + (size_t)k * ne + nx + j, 0.0);
        double v = 2.0 * c.Qs[j] * z[(size_t)k * ne + nx + j];
        if (k)
            for (int r = 0; r < mc; ++r)
                if (c.row_slack[r] == j) v += c.row_sign[r] * yg((k - 1) * mc + r);
        res = nmax(res, fabs(v));
    }

    // ---- the costate chain ----
    const bool xl = t < nx, ul = t >= nx && t < nx + nu;
    const int ju = t - nx;
    double Qrow[CMPC_MAX_NX];
#pragma unroll
    for (int u = 0; u < CMPC_MAX_NX; ++u) Qrow[u] = (xl && u < nx) ? c.Q[t * nx + u] : 0.0;
    // what stage k subtracts from [A_k B_k]' nu_{k+1}: g_k on the state lanes, the u column's own terms
    // 2 R u_k + y_ub - y_lb + 2 dR du_k - 2 dR du_{k+1} on the input lanes (k < N), 0 elsewhere
    auto side_of = [&](int k) -> double {
        const double xk = xl ? z[(size_t)k * ne + t] : 0.0;
        double gq = 0.0;
        static_for<0, CMPC_MAX_NX>([&](auto J) {
            constexpr int u = decltype(J)::value;
            if (u < nx) gq = fma(Qrow[u], bcast16<u>(xk), gq);
        });
        double g = xl ? 2.0 * gq + 2.0 * gp[(size_t)k * nx + t] : 0.0;
        if (k >= 1 && mc > 0) {
            const double* Ck = gC + (size_t)(k - 1) * mc * nx;
            const double lk = t < mc ? yg((k - 1) * mc + t) : 0.0;
            double gc = 0.0;
            static_for<0, CMPC_MAX_MC>([&](auto J) {
                constexpr int r = decltype(J)::value;
                if (r < mc) gc = fma(xl ? Ck[r * nx + t] : 0.0, bcast16<r>(lk), gc);
            });
            g += gc;
        }
        if (ul && k < N) {
            double ru = 0.0;
            for (int e = 0; e < nu; ++e) ru = fma(c.R[ju * nu + e], zu[k * nu + e], ru);
            const int r0 = ms + 2 * (k * nu + ju);
            g = 2.0 * ru + yg(r0) - yg(r0 + 1) + 2.0 * drdu(k, ju);
            if (k + 1 < N) g -= 2.0 * drdu(k + 1, ju);
        }
        return g;
    };
    auto coef_of = [&](int k, double (&M)[CMPC_MAX_NX]) {
        const double* Ak = gA + (size_t)k * nx * nx;
        const double* Bk = gB + (size_t)k * nx * nu;
#pragma unroll
        for (int j = 0; j < CMPC_MAX_NX; ++j) {
            double v = 0.0;
            if (j < nx) {
                if (xl) v = Ak[j * nx + t];
                else if (ul) v = Bk[j * nu + ju];
            }
            M[j] = v;
        }
    };
    double nuv = -side_of(N);  // nu_N = -g_N (0 past the state lanes)
    if (xl) put((size_t)m + (size_t)N * ne + t, nuv);
    double Mn[CMPC_MAX_NX];
    coef_of(N - 1, Mn);
    double side_n = side_of(N - 1);
    for (int k = N - 1; k >= 0; --k) {
        double M[CMPC_MAX_NX];
#pragma unroll
        for (int j = 0; j < CMPC_MAX_NX; ++j) M[j] = Mn[j];
        const double side = side_n;
        if (k > 0) {  // stage k - 1's operands, before this stage's chain is consumed
            coef_of(k - 1, Mn);
            side_n = side_of(k - 1);
        }
        double acc = 0.0;
        static_for<0, CMPC_MAX_NX>([&](auto J) {
            constexpr int j = decltype(J)::value;
            if (j < nx) acc = fma(M[j], bcast16<j>(nuv), acc);
        });
        const double out = acc - side;
        // state lanes: nu_k, and the x column's rounding residual; input lanes: minus the u column's residual
        const double rx = (side + out) - acc;
        res = nmax(res, xl ? fabs(rx) : (ul ? fabs(out) : 0.0));
        nuv = xl ? out : 0.0;
        if (xl) put((size_t)m + (size_t)k * ne + t, nuv);
    }
    res = row_reduce(res, nmax_);
    if (live && t == 0 && P.dua_res) P.dua_res[b] = ok ? res : qnan;
}

}  // namespace

hipError_t mpc_dual_launch(const MpcConst& c, const MpcPtrs& p, const double* z, const double* lam,
                           unsigned long long lam_stride, const double* valid, unsigned long long valid_stride,
                           double* y, double* dua_res, int batch, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    const DualPtrs d{p.A, p.B, p.p, p.C, p.h, z, lam, valid, lam_stride, valid_stride, y, dua_res};
    const int per = kDualThreads / kRow;
    hipLaunchKernelGGL(mpc_dual_kernel, dim3((batch + per - 1) / per), dim3(kDualThreads), 0, s, c, d, batch);
    return hipGetLastError();
}

}  // namespace cmpc
