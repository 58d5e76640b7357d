// Consensus rounds for any linear agent model (include/cmpc.h, cmpc_lin_*): the per-round rebuild and the
// round advance of an agent given by its own stage rows C_own / h_own (mo per stage), its own linear cost
// qlin_own and the two state columns ix, iy of its position.  The builder is di_stage_rows (di_rows.h) with
// the four constant rows and the two constant cost entries moved into the caller's arrays: the hyperplane
// arithmetic of compute_plane.py:41-68 and the coverage weights of misc.py:10-18 in the same operation
// order, so the double-integrator family is the special case ix, iy = 0, 1, mo = 4, bit for bit.
//   rows per stage k=1..N  [ C_own rows (mo) ; a_i . p <= -d/2 - b_i  (i < nb) ]
//   planes from row k-1 of the previous trajectories, weights from row k
//   p_k = qlin_own_k + wq sum_i w_i a_i on (ix, iy)
// One workgroup (one wavefront) per agent, no LDS, no scratch: the copies go lane by lane over consecutive
// addresses, the planes one lane per stage with the neighbours in order.
// lin_table_build_kernel (cmpc_lin_table_build_dev) is the same build for an agent whose future is a stage table:
// the own data of window stage k come from table row row(t + k), and the A / B windows go out in the same launch.
// lin_publish_kernel (cmpc_lin_publish_dev) is the advance's trajectory part for an inner round of a consensus
// step: it publishes the predicted positions and tests them against the ones published before.
// Every kernel is a template on the position dimension PD: 2 is the planar family (traj x 2, columns ix, iy), 3 the
// cmpc_lin3_* entries (traj x 3, columns ix, iy, iz: the third coordinate joins the distance, the normal and the
// coverage term).  The launches pick the instantiation by LinConst::pos_dim().
#include <cmath>

#include "internal.h"
#include "publish.h"
#include "wave_ops.h"

namespace cmpc {

namespace {

// Stage k = 1..N of one agent: the nb planes (row k-1 of the trajectories) into rows mo.. of C / h at row index
// k-1, and the coverage term (row k) added to the own cost row `qk` of that stage.  The one statement of the
// family's arithmetic: lin_build_kernel and lin_table_build_kernel differ only in where `qk` comes from.
template <int PD>
__device__ __forceinline__ void lin_stage(const LinConst& c, const double* traj_all, const double* own, const int* nbr,
                                          int k, const double* qk, double* qlin, double* C, double* h) {
#pragma clang fp contract(off)
    const int N = c.N, nx = c.nx, mo = c.mo, nb = c.nb, mc = mo + nb, ix = c.ix, iy = c.iy;
    const int h1 = k - 1;
    double* Ck = C + ((size_t)h1 * mc + mo) * nx;
    double* hk = h + (size_t)h1 * mc + mo;
    if constexpr (PD == 3) {
        // the planar statement below with the third coordinate in every sum, left to right
        const int iz = c.iz;
        double px = 0.0, py = 0.0, pz = 0.0;
        for (int i = 0; i < nb; ++i) {
            const double* nt = traj_all + (size_t)nbr[i] * (N + 1) * 3;
            const double ex = own[h1 * 3], ey = own[h1 * 3 + 1], ez = own[h1 * 3 + 2];
            const double nx_ = nt[h1 * 3], ny_ = nt[h1 * 3 + 1], nz_ = nt[h1 * 3 + 2];
            const double dx = nx_ - ex, dy = ny_ - ey, dz = nz_ - ez;
            const double nrm = sqrt(dx * dx + dy * dy + dz * dz);
            const double ax = dx / nrm, ay = dy / nrm, az = dz / nrm;
            const double bb = -0.5 * (ax * (ex + nx_) + ay * (ey + ny_) + az * (ez + nz_));
            const double qx = own[k * 3] - nt[k * 3], qy = own[k * 3 + 1] - nt[k * 3 + 1],
                         qz = own[k * 3 + 2] - nt[k * 3 + 2];
            const double wgt = (2.0 * c.min_dist - sqrt(qx * qx + qy * qy + qz * qz)) / nb;
            Ck[(size_t)i * nx + ix] = ax;
            Ck[(size_t)i * nx + iy] = ay;
            Ck[(size_t)i * nx + iz] = az;
            hk[i] = -c.min_dist / 2 - bb;
            px = px + c.wq * wgt * ax;
            py = py + c.wq * wgt * ay;
            pz = pz + c.wq * wgt * az;
        }
        qlin[(size_t)k * nx + ix] = qk[ix] + px;
        qlin[(size_t)k * nx + iy] = qk[iy] + py;
        qlin[(size_t)k * nx + iz] = qk[iz] + pz;
        return;
    }
    double px = 0.0, py = 0.0;
    for (int i = 0; i < nb; ++i) {
        const double* nt = traj_all + (size_t)nbr[i] * (N + 1) * 2;
        const double ex = own[h1 * 2], ey = own[h1 * 2 + 1];
        const double nx_ = nt[h1 * 2], ny_ = nt[h1 * 2 + 1];
        const double dx = nx_ - ex, dy = ny_ - ey;
        const double nrm = sqrt(dx * dx + dy * dy);
        const double ax = dx / nrm, ay = dy / nrm;
        const double bb = -0.5 * (ax * (ex + nx_) + ay * (ey + ny_));
        const double qx = own[k * 2] - nt[k * 2], qy = own[k * 2 + 1] - nt[k * 2 + 1];
        const double wgt = (2.0 * c.min_dist - sqrt(qx * qx + qy * qy)) / nb;
        Ck[(size_t)i * nx + ix] = ax;
        Ck[(size_t)i * nx + iy] = ay;
        hk[i] = -c.min_dist / 2 - bb;
        px = px + c.wq * wgt * ax;
        py = py + c.wq * wgt * ay;
    }
    qlin[(size_t)k * nx + ix] = qk[ix] + px;
    qlin[(size_t)k * nx + iy] = qk[iy] + py;
}

// state column s holds a position coordinate (the stage lanes write those entries of stages 1..N)
template <int PD>
__device__ __forceinline__ bool is_pos(const LinConst& c, int s) {
    return s == c.ix || s == c.iy || (PD == 3 && s == c.iz);
}

template <int PD>
__global__ __launch_bounds__(kWave) void lin_build_kernel(const LinConst c, const LinPtrs P) {
#pragma clang fp contract(off)
    const int b = blockIdx.x;
    const int N = c.N, nx = c.nx, mo = c.mo, nb = c.nb, mc = mo + nb;
    const double* own = P.traj_all + (size_t)(c.self_offset + b) * (N + 1) * PD;
    const int* nbr = P.nbr + (size_t)b * nb;
    const double* qo = P.qlin_own + (size_t)b * (N + 1) * nx;
    const double* Co = P.C_own + (size_t)b * N * mo * nx;  // (not dereferenced when mo == 0)
    const double* ho = P.h_own + (size_t)b * N * mo;
    double* qlin = P.qlin + (size_t)b * (N + 1) * nx;
    double* C = P.C + (size_t)b * N * mc * nx;
    double* h = P.h + (size_t)b * N * mc;

    // the own cost, except the two position entries of stages 1..N (the stage lanes below write those)
    for (int i = threadIdx.x; i < (N + 1) * nx; i += kWave) {
        const int s = i % nx;
        if (i < nx || !is_pos<PD>(c, s)) qlin[i] = qo[i];
    }
    // the own rows, and the zeros of the plane rows (their ix, iy entries: the stage lanes)
    for (int i = threadIdx.x; i < N * mc * nx; i += kWave) {
        const int s = i % nx, kr = i / nx, r = kr % mc, k1 = kr / mc;
        if (r < mo)
            C[i] = Co[((size_t)k1 * mo + r) * nx + s];
        else if (!is_pos<PD>(c, s))
            C[i] = 0.0;
    }
    for (int i = threadIdx.x; i < N * mc; i += kWave) {
        const int r = i % mc, k1 = i / mc;
        if (r < mo) h[i] = ho[(size_t)k1 * mo + r];
    }
    // stage k = 1..N: the nb planes (row k-1 of the trajectories) and the coverage term (row k)
    for (int k = threadIdx.x + 1; k <= N; k += kWave)
        lin_stage<PD>(c, P.traj_all, own, nbr, k, qo + (size_t)k * nx, qlin, C, h);
}

// The stage table's row of window stage k at time t (include/cmpc.h, "stage table"): tau = t + k fits an int
// (the entry point checks t <= INT_MAX - N)
__device__ __forceinline__ size_t table_row(const LinTableConst& tc, int k) {
    const int tau = tc.t + k;
    return tc.mode == CMPC_TABLE_PERIODIC ? (size_t)(tau % tc.T) : (size_t)(tau < tc.T ? tau : tc.T - 1);
}

// lin_build_kernel with the own data read through table_row straight from the stage table, and the A / B
// windows of the round copied into the solver's arrays by the same launch
template <int PD>
__global__ __launch_bounds__(kWave) void lin_table_build_kernel(const LinConst c, const LinTableConst tc,
                                                                const LinTablePtrs P) {
#pragma clang fp contract(off)
    const int b = blockIdx.x;
    const int N = c.N, nx = c.nx, mo = c.mo, nb = c.nb, mc = mo + nb;
    const size_t T = (size_t)tc.T, nA = (size_t)nx * nx, nB = (size_t)nx * tc.nu;
    const double* own = P.traj_all + (size_t)(c.self_offset + b) * (N + 1) * PD;
    const int* nbr = P.nbr + (size_t)b * nb;
    const double* At = P.A_tab + (size_t)b * T * nA;
    const double* Bt = P.B_tab + (size_t)b * T * nB;
    const double* qt = P.qlin_tab + (size_t)b * T * nx;
    const double* Ct = P.C_tab + (size_t)b * T * mo * nx;  // (not dereferenced when mo == 0)
    const double* ht = P.h_tab + (size_t)b * T * mo;
    double* A = P.A + (size_t)b * N * nA;
    double* B = P.B + (size_t)b * N * nB;
    double* qlin = P.qlin + (size_t)b * (N + 1) * nx;
    double* C = P.C + (size_t)b * N * mc * nx;
    double* h = P.h + (size_t)b * N * mc;

    // the model's window: stages t .. t+N-1
    for (size_t i = threadIdx.x; i < (size_t)N * nA; i += kWave) A[i] = At[table_row(tc, (int)(i / nA)) * nA + i % nA];
    for (size_t i = threadIdx.x; i < (size_t)N * nB; i += kWave) B[i] = Bt[table_row(tc, (int)(i / nB)) * nB + i % nB];
    // the own cost of stages t .. t+N, except the two position entries of window stages 1..N (the stage lanes)
    for (size_t i = threadIdx.x; i < (size_t)(N + 1) * nx; i += kWave) {
        const int s = (int)(i % nx), k = (int)(i / nx);
        if (k == 0 || !is_pos<PD>(c, s)) qlin[i] = qt[table_row(tc, k) * nx + s];
    }
    // the own rows of stages t+1 .. t+N, and the zeros of the plane rows
    for (size_t i = threadIdx.x; i < (size_t)N * mc * nx; i += kWave) {
        const int s = (int)(i % nx), r = (int)(i / nx % mc), k1 = (int)(i / nx / mc);
        if (r < mo)
            C[i] = Ct[(table_row(tc, k1 + 1) * mo + r) * nx + s];
        else if (!is_pos<PD>(c, s))
            C[i] = 0.0;
    }
    for (size_t i = threadIdx.x; i < (size_t)N * mc; i += kWave) {
        const int r = (int)(i % mc), k1 = (int)(i / mc);
        if (r < mo) h[i] = ht[table_row(tc, k1 + 1) * mo + r];
    }
    for (int k = threadIdx.x + 1; k <= N; k += kWave)
        lin_stage<PD>(c, P.traj_all, own, nbr, k, qt + table_row(tc, k) * nx, qlin, C, h);
}

// x0 <- x_1, u_prev <- u_0, traj <- predicted (z[ix], z[iy]) (PD = 3: and z[iz]) for k = 0..N  (z in reference
// layout); an agent with a non-finite z keeps all three (no NaN reaches a neighbour: the LPV advance's rule)
template <int PD>
__global__ __launch_bounds__(kWave) void lin_advance_kernel(const LinConst c, int ns, int nu,
                                                            const double* __restrict__ z, double* x0, double* up,
                                                            double* traj) {
    const int b = blockIdx.x;
    const int N = c.N, nx = c.nx, nxe = nx + ns;
    const size_t nz = (size_t)nxe * (N + 1) + 2 * (size_t)nu * N;
    const double* zb = z + (size_t)b * nz;
    bool bad = false;
    for (size_t i = threadIdx.x; i < nz; i += kWave) bad |= !isfinite(zb[i]);
    if (__any(bad)) return;  // (the workgroup is one wavefront)
    if constexpr (PD == 2) {
        for (int i = threadIdx.x; i < 2 * (N + 1); i += kWave) {
            const int k = i >> 1;
            traj[(size_t)b * 2 * (N + 1) + i] = zb[(size_t)k * nxe + ((i & 1) ? c.iy : c.ix)];
        }
    } else {
        for (int i = threadIdx.x; i < 3 * (N + 1); i += kWave) {
            const int k = i / 3, a = i - 3 * k;
            traj[(size_t)b * 3 * (N + 1) + i] = zb[(size_t)k * nxe + (a == 0 ? c.ix : a == 1 ? c.iy : c.iz)];
        }
    }
    if ((int)threadIdx.x < nx) x0[(size_t)b * nx + threadIdx.x] = zb[nxe + threadIdx.x];
    if ((int)threadIdx.x < nu) up[(size_t)b * nu + threadIdx.x] = zb[(size_t)nxe * (N + 1) + threadIdx.x];
}

// An inner round's publication (include/cmpc.h, cmpc_lin_publish_dev): traj_local <- predicted (z[ix], z[iy]) and
// the allclose test of it against the agent's row of the exchange buffer; an agent with a non-finite z publishes
// that row again and is never close.  The rule is publish_agent's (publish.h), shared with the LPV family's kernel.
template <int PD>
__global__ __launch_bounds__(kWave) void lin_publish_kernel(const LinConst c, int ns, int nu, double atol, double rtol,
                                                            const double* __restrict__ z,
                                                            const double* __restrict__ traj_all,
                                                            double* __restrict__ traj_local, int* close, double* delta,
                                                            int* not_close) {
    const int b = blockIdx.x;
    const int N = c.N, nxe = c.nx + ns, per = PD * (N + 1);
    const size_t nz = (size_t)nxe * (N + 1) + 2 * (size_t)nu * N;
    publish_agent<PD>(z + (size_t)b * nz, nz, nxe, c.ix, c.iy, per, traj_all + (size_t)(c.self_offset + b) * per,
                      traj_local + (size_t)b * per, atol, rtol, close ? close + b : nullptr,
                      delta ? delta + b : nullptr, not_close, c.iz);
}

}  // namespace

hipError_t lin_build_launch(const LinConst& c, const LinPtrs& p, int batch, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    if (c.pos_dim() == 3)
        hipLaunchKernelGGL(lin_build_kernel<3>, dim3(batch), dim3(kWave), 0, s, c, p);
    else
        hipLaunchKernelGGL(lin_build_kernel<2>, dim3(batch), dim3(kWave), 0, s, c, p);
    return hipGetLastError();
}

hipError_t lin_table_build_launch(const LinConst& c, const LinTableConst& tc, const LinTablePtrs& p, int batch,
                                  hipStream_t s) {
    if (batch == 0) return hipSuccess;
    if (c.pos_dim() == 3)
        hipLaunchKernelGGL(lin_table_build_kernel<3>, dim3(batch), dim3(kWave), 0, s, c, tc, p);
    else
        hipLaunchKernelGGL(lin_table_build_kernel<2>, dim3(batch), dim3(kWave), 0, s, c, tc, p);
    return hipGetLastError();
}

hipError_t lin_advance_launch(const LinConst& c, int ns, int nu, const double* z, double* x0, double* up,
                              double* traj, int batch, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    if (c.pos_dim() == 3)
        hipLaunchKernelGGL(lin_advance_kernel<3>, dim3(batch), dim3(kWave), 0, s, c, ns, nu, z, x0, up, traj);
    else
        hipLaunchKernelGGL(lin_advance_kernel<2>, dim3(batch), dim3(kWave), 0, s, c, ns, nu, z, x0, up, traj);
    return hipGetLastError();
}

hipError_t lin_publish_launch(const LinConst& c, int ns, int nu, double atol, double rtol, const double* z,
                              const double* traj_all, double* traj_local, int* close, double* delta, int* not_close,
                              int batch, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    if (c.pos_dim() == 3)
        hipLaunchKernelGGL(lin_publish_kernel<3>, dim3(batch), dim3(kWave), 0, s, c, ns, nu, atol, rtol, z, traj_all,
                           traj_local, close, delta, not_close);
    else
        hipLaunchKernelGGL(lin_publish_kernel<2>, dim3(batch), dim3(kWave), 0, s, c, ns, nu, atol, rtol, z, traj_all,
                           traj_local, close, delta, not_close);
    return hipGetLastError();
}

}  // namespace cmpc
