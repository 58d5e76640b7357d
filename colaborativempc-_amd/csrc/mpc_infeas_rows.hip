// Primal-infeasibility certificate of the structured agent QP for infeasibility that needs several hard rows
// combined (cmpc.h, cmpc_mpc_cert_rows; the numpy statement is cmpc.infeas.certify_rows).
//
// H: the hard stage rows (row_slack[r] == -1) of finite h.  The rows of H, the dynamics and the input box are
// infeasible together exactly when the least-squares violation  min over the box of 1/2 ||(C x(u) - h)_+||^2  is
// positive, and at its minimiser the violation vector is a Farkas ray.  FISTA (no restart, no line search) with
// the step 1 / Lf, Lf = the squared Frobenius norm of u -> (row values), proposes; every check_every iterations
// the violation vector at u, w = v / max v, weights the rows into one aggregated row, whose reachability over the
// box (the test of mpc_infeas.hip, same sums, same threshold) alone decides:
//   P_N = C_N' w_N,  P_j = C_j' w_j + A_j' P_{j+1},  P_0 = A_0' P_1,  g_j = B_j' P_{j+1}
//   reach = P_0'x0 + sum min(g_ji lb_i, g_ji ub_i),  S = sum |w h| + sum |P_0s x0_s| + sum |g_ji| |that bound|
//   certified when no touched bound is infinite and reach - w'h > kCertTol S.
// The ray (cmpc_mpc_duals.y layout): w on the stage rows, t = -g_ji split by sign onto input i's two box rows,
// nu_j = -P_j on the state rows, 0 on the slack and input-rate rows.
//
// Layout: one wavefront per agent; an agent at status 1, 2 or -3 returns at once.  The iterates u and y (N nu each)
// and the violation vector (N mc) live in LDS.  A, B, C, h are read in every pass, one stage ahead of the
// arithmetic: from an LDS copy made once where the agent's stage data fits beside the iterates (STAGED; the
// measured gain is in DESIGN section 3), from global memory and L2 at any other horizon (N = 125 at nx = 9).  The stage recursions are
// sequential.  Forward: lane s holds x[s] and row s of A_j and B_j, lane r row r of C_j; the state is broadcast
// lane by lane (v_readlane).  Backward: lane t holds P[t] and column t of C_j and A_j, lane i column i of B_j and
// input i's accumulators.  Register arrays are indexed statically only.  Lf pre-pass: lanes own rows of H in
// passes of 64, the recursion of mpc_infeas.hip.  NaN or infinite data falls through every comparison to "no
// certificate".  Every element of an output row is written exactly once.
#include "infeas_ops.h"
#include "internal.h"
#include "wave_ops.h"

namespace cmpc {
namespace {

struct RowsPtrs {
    const double* __restrict__ A;
    const double* __restrict__ B;
    const double* __restrict__ x0;
    const double* __restrict__ C;
    const double* __restrict__ h;
    int* status;     // in-out, optional
    double* ray;     // optional
    double* margin;  // optional
    int* iters;      // optional
    int* nrows;      // optional
    int max_iter, check_every;
};

// lb where v < lb, ub where the result > ub: a NaN bound never clips, a NaN v stays
__device__ __forceinline__ double clip(double v, double lb, double ub) {
    v = v < lb ? lb : v;
    return v > ub ? ub : v;
}

// The passes are instantiated on their loop bounds KX >= nx, KU >= nu, KM >= mc: the library's limits (any
// dimension the API accepts), or the very dimensions of the common models, whose masks and clamps then fold away.
// one stage's operands of the forward pass, as lane `lane` holds them
template <int KX, int KU, int KM>
struct FwdStage {
    double a[KX], b[KU], c[KX], h;
};
// ... and of the backward pass
template <int KX, int KU, int KM>
struct BwdStage {
    double c[KM], a[KX], b[KX], h;
};

struct Agent {
    int lane, nx, nu, N, mc;
    const double *gA, *gB, *gC, *gh;  // the stage data: global memory, or its LDS copy
    double x0;        // lane < nx: x0[lane], else 0
    unsigned hmask;   // bit r: row r is hard
    bool hard;        // lane < mc and row `lane` is hard
    double lb, ub;    // lane < nu: input `lane`'s bounds
    double *U, *Y, *V;  // LDS: N nu, N nu, N mc
};

// Every load below is unconditional at a clamped (valid) index and masked afterwards: the compiler turns a guarded
// load into a branch with its own wait, some 50 of them per stage
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

template <int KX, int KU, int KM>
__device__ __forceinline__ FwdStage<KX, KU, KM> load_fwd(const Agent& a, int j) {
    FwdStage<KX, KU, KM> f;
    const int l = a.lane, ls = imin(l, a.nx - 1), lr = imin(l, a.mc - 1);
    const double* Aj = a.gA + (size_t)j * a.nx * a.nx + ls * a.nx;
    const double* Bj = a.gB + (size_t)j * a.nx * a.nu + ls * a.nu;
    const double* Cj = a.gC + ((size_t)j * a.mc + lr) * a.nx;
#pragma unroll
    for (int t = 0; t < KX; ++t) {
        const int tc = imin(t, a.nx - 1);
        const double av = Aj[tc], cv = Cj[tc];
        f.a[t] = (l < a.nx && t < a.nx) ? av : 0.0;
        f.c[t] = (l < a.mc && t < a.nx) ? cv : 0.0;
    }
#pragma unroll
    for (int i = 0; i < KU; ++i) {
        const double bv = Bj[imin(i, a.nu - 1)];
        f.b[i] = (l < a.nx && i < a.nu) ? bv : 0.0;
    }
    const double hv = a.gh[(size_t)j * a.mc + lr];
    f.h = l < a.mc ? hv : 0.0;
    return f;
}

template <int KX, int KU, int KM>
__device__ __forceinline__ BwdStage<KX, KU, KM> load_bwd(const Agent& a, int j) {
    BwdStage<KX, KU, KM> f;
    const int l = a.lane, lt = imin(l, a.nx - 1), li = imin(l, a.nu - 1);
    const double* Aj = a.gA + (size_t)j * a.nx * a.nx + lt;
    const double* Bj = a.gB + (size_t)j * a.nx * a.nu + li;
    const double* Cj = a.gC + (size_t)j * a.mc * a.nx + lt;
#pragma unroll
    for (int r = 0; r < KM; ++r) {
        const double cv = Cj[imin(r, a.mc - 1) * a.nx];
        f.c[r] = (l < a.nx && ((a.hmask >> r) & 1)) ? cv : 0.0;
    }
#pragma unroll
    for (int s = 0; s < KX; ++s) {
        const int sc = imin(s, a.nx - 1);
        const double av = Aj[sc * a.nx], bv = Bj[sc * a.nu];
        f.a[s] = (l < a.nx && s < a.nx) ? av : 0.0;
        f.b[s] = (l < a.nu && s < a.nx) ? bv : 0.0;
    }
    const double hv = a.gh[(size_t)j * a.mc + imin(l, a.mc - 1)];
    f.h = l < a.mc ? hv : 0.0;
    return f;
}

// x forward from x0 with the inputs `in` (LDS); V <- max(C x - h, 0) on H, 0 elsewhere (a NaN stays); returns
// its largest entry (NaN when any is NaN), the same on every lane
template <int KX, int KU, int KM>
__device__ __forceinline__ double forward(const Agent& a, const double* in) {
    const int l = a.lane;
    double xs[KX];
#pragma unroll
    for (int t = 0; t < KX; ++t) xs[t] = readlane_d(a.x0, t);  // (lanes nx .. hold 0)
    double vmax = 0.0;
    FwdStage<KX, KU, KM> cur = load_fwd<KX, KU, KM>(a, 0);
    for (int j = 0; j < a.N; ++j) {
        const FwdStage<KX, KU, KM> nxt = load_fwd<KX, KU, KM>(a, j + 1 < a.N ? j + 1 : j);
        double xn = 0.0;
#pragma unroll
        for (int t = 0; t < KX; ++t) xn = fma(cur.a[t], xs[t], xn);
#pragma unroll
        for (int i = 0; i < KU; ++i) {
            const double ui = in[j * a.nu + imin(i, a.nu - 1)];
            xn = fma(cur.b[i], i < a.nu ? ui : 0.0, xn);
        }
        xn = l < a.nx ? xn : 0.0;  // (0 * inf: the idle lanes stay 0)
#pragma unroll
        for (int t = 0; t < KX; ++t) xs[t] = readlane_d(xn, t);
        double cv = 0.0;
#pragma unroll
        for (int t = 0; t < KX; ++t) cv = fma(cur.c[t], xs[t], cv);
        cv -= cur.h;
        const double v = (a.hard && isfinite(cur.h)) ? nmax(cv, 0.0) : 0.0;
        if (l < a.mc) a.V[j * a.mc + l] = v;
        vmax = nmax(vmax, v);
        cur = nxt;
    }
    wsync();
    return wave_max(vmax);
}

enum { kStep = 0, kCheck = 1, kWrite = 2 };

struct CheckSums {
    double reach, S, wh;  // this lane's share
    int rows;
    bool disq;
};

// The backward recursion on the weights V / mw (kStep: mw = 1, no division).
//  kStep:  u+ = clip(y - g step), y <- u+ + beta (u+ - u), u <- u+
//  kCheck: the aggregated row's sums into cs (each lane its share)
//  kWrite: the ray row y (stage rows, box rows, state rows)
template <int MODE, int KX, int KU, int KM>
__device__ __forceinline__ void backward(const Agent& a, double mw, double step, double beta,
                                         CheckSums& cs, double* y, int ms, int m, int ne) {
    const int l = a.lane;
    double P = 0.0;
    BwdStage<KX, KU, KM> cur = load_bwd<KX, KU, KM>(a, a.N - 1);
    for (int j = a.N - 1; j >= 0; --j) {
        const BwdStage<KX, KU, KM> nxt = load_bwd<KX, KU, KM>(a, j > 0 ? j - 1 : 0);
#pragma unroll
        for (int r = 0; r < KM; ++r) {
            double vr = a.V[j * a.mc + imin(r, a.mc - 1)];
            if (MODE != kStep) vr = vr / mw;
            // (a soft row never counts; the idle lanes stay 0)
            P = (((a.hmask >> r) & 1) && l < a.nx && vr != 0.0) ? fma(cur.c[r], vr, P) : P;
        }
        if (MODE != kStep) {
            const double wl = l < a.mc ? a.V[j * a.mc + imin(l, a.mc - 1)] / mw : 0.0;  // (0 off H)
            if (MODE == kCheck) {
                const bool nz = wl != 0.0;
                const double whv = nz ? wl * cur.h : 0.0;
                cs.wh += whv;
                cs.S += fabs(whv);
                cs.rows += nz ? 1 : 0;
            } else {
                if (l < a.mc) y[(size_t)j * a.mc + l] = wl;
                if (l < a.nx) y[(size_t)m + (size_t)(j + 1) * ne + l] = -P;
            }
        }
        double ps[KX];
#pragma unroll
        for (int s = 0; s < KX; ++s) ps[s] = readlane_d(P, s);
        double g = 0.0, pn = 0.0;
#pragma unroll
        for (int s = 0; s < KX; ++s) {
            g = fma(cur.b[s], ps[s], g);
            pn = fma(cur.a[s], ps[s], pn);
        }
        P = l < a.nx ? pn : 0.0;
        if (l < a.nu) {
            if (MODE == kStep) {
                const int e = j * a.nu + l;
                const double uo = a.U[e];
                const double un = clip(a.Y[e] - g * step, a.lb, a.ub);
                a.U[e] = un;
                a.Y[e] = un + beta * (un - uo);
            } else if (MODE == kCheck) {
                const double bnd = g > 0.0 ? a.lb : a.ub;
                const bool term = g != 0.0;  // (a NaN g is a term: it poisons reach)
                const bool fin = isfinite(bnd);
                cs.disq = cs.disq || (term && !fin);
                cs.reach += (term && fin) ? g * bnd : 0.0;
                cs.S += (term && fin) ? fabs(g) * fabs(bnd) : 0.0;
            } else {
                const double t = -g;
                const size_t r0 = (size_t)ms + 2 * ((size_t)j * a.nu + l);
                y[r0] = t > 0.0 ? t : 0.0;
                y[r0 + 1] = t < 0.0 ? -t : 0.0;
            }
        }
        cur = nxt;
    }
    if (MODE == kCheck && l < a.nx) {
        const double v = P * a.x0;
        cs.reach += v;
        cs.S += fabs(v);
    }
    if (MODE == kWrite && l < a.nx) y[(size_t)m + l] = -P;
    wsync();
}

// Lf = sum over H of sum_{j<k, i} g_ji^2 (every lane the same value); *any: H is not empty
__device__ __forceinline__ double lipschitz(const Agent& a, const MpcConst& c, int nh, bool* any) {
    const int ncand = a.N * nh;
    double lf = 0.0, cnt = 0.0;
    for (int q0 = 0; q0 < ncand; q0 += kWave) {
        const int q = q0 + a.lane;
        const bool in = q < ncand;
        const int qq = in ? q : q0;  // a lane past the end redoes the pass's first row and drops it
        const int ks = qq / nh;      // stage k = ks + 1
        const int r = hard_row(c, qq - ks * nh);
        const bool use = in && isfinite(a.gh[ks * a.mc + r]);
        cnt += use ? 1.0 : 0.0;
        double p[CMPC_MAX_NX], g[CMPC_MAX_NU];
#pragma unroll
        for (int s = 0; s < CMPC_MAX_NX; ++s) p[s] = s < a.nx ? a.gC[((size_t)ks * a.mc + r) * a.nx + s] : 0.0;
        const int last = q0 + kWave - 1 < ncand ? q0 + kWave - 1 : ncand - 1;
        for (int j = last / nh; j >= 0; --j) {
            const bool on = j <= ks;
            adjoint_step(a.nx, a.nu, a.gA + (size_t)j * a.nx * a.nx, a.gB + (size_t)j * a.nx * a.nu, p, g, on);
#pragma unroll
            for (int i = 0; i < CMPC_MAX_NU; ++i)
                if (i < a.nu) lf += (use && on) ? g[i] * g[i] : 0.0;
        }
    }
    *any = wave_sum(cnt) > 0.0;
    return wave_sum(lf);
}

// dst (LDS) <- src (global), count >= 1 doubles: eight loads in flight per lane
__device__ __forceinline__ void stage_in(double* dst, const double* __restrict__ src, int count, int lane) {
    for (int e0 = 0; e0 < count; e0 += 8 * kWave) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = src[imin(e0 + q * kWave + lane, count - 1)];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (e0 + q * kWave + lane < count) dst[e0 + q * kWave + lane] = v[q];
    }
}

// FIXED: nx, nu, mc are KX, KU, KM (the launch checks it)
template <bool STAGED, bool FIXED, int KX, int KU, int KM>
__global__ __launch_bounds__(kWave) void mpc_infeas_rows_kernel(const MpcConst c, const RowsPtrs P) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    if (P.status) {
        const int st = P.status[b];  // (the whole wave: one agent)
        if (st == CMPC_SOLVED || st == CMPC_SOLVED_INACCURATE || st == CMPC_PRIMAL_INFEASIBLE) return;
    }
    const int nx = FIXED ? KX : c.nx, nu = FIXED ? KU : c.nu, mc = FIXED ? KM : c.mc;
    const int N = c.N, ns = c.ns, ms = c.ms, m = c.m, n = c.n;
    const int ne = nx + ns;
    const double qnan = __builtin_nan("");
    Agent a;
    a.lane = lane, a.nx = nx, a.nu = nu, a.N = N, a.mc = mc;
    a.gA = P.A + b * N * nx * nx;
    a.gB = P.B + b * N * nx * nu;
    a.gC = P.C + b * N * mc * nx;
    a.gh = P.h + b * N * mc;
    a.x0 = lane < nx ? P.x0[b * nx + lane] : 0.0;
    a.U = lds, a.Y = lds + n, a.V = lds + 2 * n;
    if (STAGED) {  // the agent's stage data, once
        double* sA = lds + 2 * n + ms;
        double* sB = sA + N * nx * nx;
        double* sC = sB + N * nx * nu;
        double* sh = sC + ms * nx;
        stage_in(sA, a.gA, N * nx * nx, lane);
        stage_in(sB, a.gB, N * nx * nu, lane);
        stage_in(sC, a.gC, ms * nx, lane);
        stage_in(sh, a.gh, ms, lane);
        a.gA = sA, a.gB = sB, a.gC = sC, a.gh = sh;
        wsync();
    }
    a.hmask = 0, a.hard = false, a.lb = 0.0, a.ub = 0.0;
    bool box = true;  // u_lb <= u_ub on every input (a NaN bound passes here and disqualifies its terms below)
    int nh = 0;
#pragma unroll
    for (int r = 0; r < CMPC_MAX_MC; ++r) {
        if (r < mc && c.row_slack[r] < 0) {
            ++nh;
            a.hmask |= 1u << r;
            a.hard = lane == r ? true : a.hard;
        }
    }
#pragma unroll
    for (int i = 0; i < CMPC_MAX_NU; ++i) {
        if (i < nu) {
            if (c.u_lb[i] > c.u_ub[i]) box = false;
            a.lb = lane == i ? c.u_lb[i] : a.lb;
            a.ub = lane == i ? c.u_ub[i] : a.ub;
        }
    }

    double margin = qnan, mw = 0.0;
    int it = 0, rows = 0;
    bool cert = false, any = false;
    double lf = 0.0;
    if (box && nh > 0) lf = lipschitz(a, c, nh, &any);
    if (any && isfinite(lf) && lf > 0.0) {
        const double step = 1.0 / lf;
        for (int e = lane; e < n; e += kWave) {  // u0 = clip(0, lb, ub), input e % nu
            const int i = e % nu;
            double lo = 0.0, hi = 0.0;
#pragma unroll
            for (int ii = 0; ii < CMPC_MAX_NU; ++ii) {
                lo = (ii < nu && i == ii) ? c.u_lb[ii] : lo;
                hi = (ii < nu && i == ii) ? c.u_ub[ii] : hi;
            }
            const double u0 = clip(0.0, lo, hi);
            a.U[e] = u0;
            a.Y[e] = u0;
        }
        wsync();
        double t = 1.0;
        CheckSums cs{};
        while (it < P.max_iter) {
            ++it;
            forward<KX, KU, KM>(a, a.Y);
            const double tn = (1.0 + sqrt(1.0 + 4.0 * t * t)) / 2.0;
            const double beta = (t - 1.0) / tn;
            t = tn;
            backward<kStep, KX, KU, KM>(a, 1.0, step, beta, cs, nullptr, ms, m, ne);
            if (it % P.check_every != 0 && it != P.max_iter) continue;
            // ---- the check: the violation at u weights the rows; the aggregated row's reachability decides ----
            mw = forward<KX, KU, KM>(a, a.U);
            if (!(mw > 0.0)) {  // every hard row holds at u (margin 0), or NaN data (no candidate)
                margin = mw == 0.0 ? 0.0 : qnan;
                rows = 0;
                break;
            }
            cs = CheckSums{};
            backward<kCheck, KX, KU, KM>(a, mw, step, 0.0, cs, nullptr, ms, m, ne);
            const double reach = wave_sum(cs.reach), S = wave_sum(cs.S), wh = wave_sum(cs.wh);
            const bool disq = wave_max(cs.disq ? 1.0 : 0.0) > 0.0;
            rows = (int)wave_sum((double)cs.rows);
            const double d = reach - wh;
            margin = disq ? qnan : d / S;
            if (!disq && d > kCertTol * S) {
                cert = true;
                break;
            }
        }
    }
    if (lane == 0) {
        if (cert && P.status) P.status[b] = CMPC_PRIMAL_INFEASIBLE;
        if (P.margin) P.margin[b] = margin;
        if (P.iters) P.iters[b] = it;
        if (P.nrows) P.nrows[b] = rows;
    }
    if (!P.ray) return;
    const size_t nxa = (size_t)ne * (N + 1), ny = (size_t)m + nxa + n;
    double* y = P.ray + b * ny;
    if (!cert) {
        for (size_t e = lane; e < ny; e += kWave) y[e] = qnan;
        return;
    }
    // ---- the ray: every element once.  The slack rows and the input-rate rows, then the recursion's rows ----
    for (size_t e = lane; e < nxa; e += kWave) {
        const int s = (int)(e % ne);
        if (s >= nx) y[m + e] = 0.0;
    }
    for (size_t e = lane; e < (size_t)n; e += kWave) y[(size_t)m + nxa + e] = 0.0;
    CheckSums cs{};
    backward<kWrite, KX, KU, KM>(a, mw, 0.0, 0.0, cs, y, ms, m, ne);
}

}  // namespace

template <bool FIXED, int KX, int KU, int KM>
static hipError_t launch_dims(bool staged, size_t lds, const MpcConst& c, const RowsPtrs& d, int batch, hipStream_t s) {
    const void* k = staged ? (const void*)mpc_infeas_rows_kernel<true, FIXED, KX, KU, KM>
                           : (const void*)mpc_infeas_rows_kernel<false, FIXED, KX, KU, KM>;
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (staged)
        hipLaunchKernelGGL((mpc_infeas_rows_kernel<true, FIXED, KX, KU, KM>), dim3(batch), dim3(kWave), lds, s, c, d);
    else
        hipLaunchKernelGGL((mpc_infeas_rows_kernel<false, FIXED, KX, KU, KM>), dim3(batch), dim3(kWave), lds, s, c, d);
    return hipGetLastError();
}

size_t mpc_infeas_rows_lds_bytes(const MpcConst& c) { return 8 * (2 * (size_t)c.n + (size_t)c.ms); }
// ... with the agent's A, B, C, h beside the iterates
static size_t staged_lds_bytes(const MpcConst& c) {
    return mpc_infeas_rows_lds_bytes(c) + 8 * (size_t)c.N * ((size_t)c.nx * c.nx + c.nx * c.nu + c.mc * c.nx + c.mc);
}

hipError_t mpc_infeas_rows_launch(const MpcConst& c, const MpcPtrs& p, int* status, double* ray, double* margin,
                                  int* iters, int* nrows, int max_iter, int check_every, int batch, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    if (mpc_infeas_rows_lds_bytes(c) > kMaxLdsBytes) return hipErrorInvalidValue;
#ifdef CMPC_ROWS_NO_STAGE  // (A/B builds: the stage data stays in global memory)
    const bool staged = false;
#else
    const bool staged = staged_lds_bytes(c) <= kMaxLdsBytes;
#endif
    const size_t lds = staged ? staged_lds_bytes(c) : mpc_infeas_rows_lds_bytes(c);
    const RowsPtrs d{p.A, p.B, p.x0, p.C, p.h, status, ray, margin, iters, nrows,
                     max_iter > 0 ? max_iter : CMPC_CERT_ROWS_MAX_ITER,
                     check_every > 0 ? check_every : CMPC_CERT_ROWS_CHECK_EVERY};
    // the common models' dimensions (double integrator, the LPV car, BASELINE cfg5) run their own instantiation
    if (c.nx == 4 && c.nu == 2 && c.mc == 6) return launch_dims<true, 4, 2, 6>(staged, lds, c, d, batch, s);
    if (c.nx == 9 && c.nu == 2 && c.mc == 6) return launch_dims<true, 9, 2, 6>(staged, lds, c, d, batch, s);
    if (c.nx == 6 && c.nu == 3 && c.mc == 6) return launch_dims<true, 6, 3, 6>(staged, lds, c, d, batch, s);
    return launch_dims<false, CMPC_MAX_NX, CMPC_MAX_NU, CMPC_MAX_MC>(staged, lds, c, d, batch, s);
}

}  // namespace cmpc
