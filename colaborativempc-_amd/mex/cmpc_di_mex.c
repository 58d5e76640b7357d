/* cmpc_di — MATLAB MEX gateway over libcmpc's round handle of the synthetic double-integrator family
 * (include/cmpc.h, cmpc_di_rounds_*): the consensus loop of BASELINE cfg2-cfg5 (what cmpc.rounds.DIRounds.step()
 * does), device-resident, for a MATLAB host that owns no device memory.
 *
 *   h = cmpc_di('rounds_create', P, D, S)            cmpc_di_rounds_create
 *   done = cmpc_di('rounds_step', h, k)              k rounds ([select,] build + solve + advance, [order,] exchange);
 *                                                    one host synchronisation, at the end
 *   [z, status, kkt, iters, x0, u_prev, nbr] = cmpc_di('rounds_read', h)      the latest round
 *   [kkt, iters, status] = cmpc_di('rounds_history', h, first, count)         B x count each, rounds counted
 *                                                    from create (0-based); S.history rounds are kept
 *   cmpc_di('rounds_log_enable', h, capacity [, flags])   cmpc_di_rounds_log_enable: a device log of the last
 *                                                    `capacity` rounds from here on; flags 1 = CMPC_LOG_SEPARATION
 *   L = cmpc_di('rounds_log', h [, first, count])    cmpc_di_rounds_log_read: rounds first .. first+count-1 (0-based,
 *                                                    counted from create; default: all the ring holds) as a struct —
 *                                                    first (scalar), state nx x B x count (x_0 of the round),
 *                                                    u nu x B x count (u_0), look_ahead, kkt, iters, status
 *                                                    B x count, solve_ms count x 1 (the whole batch's solver launch,
 *                                                    ms), and with CMPC_LOG_SEPARATION sep2, nearest B x count
 *                                                    (0-based global index of the nearest other agent)
 *   T = cmpc_di('rounds_get_traj', h)                this rank's predicted positions (host exchange)
 *   cmpc_di('rounds_set_traj', h, T)                 the gathered exchange buffer (host exchange)
 *   cmpc_di('rounds_destroy', h)
 *   id = cmpc_di('comm_id');  cmpc_di('comm_init', nranks, rank, id)   RCCL exchange (one GPU per rank)
 *
 *   P: struct — dim (2 or 3), v_ref, q_v, q_lane, hw, min_vel, max_vel, min_dist, wq (cmpc_di_params), N,
 *      the solver's weights Q nx x nx, R nu x nu, dR nu x nu, Qs 3x1, u_ub nu x 1, u_lb nu x 1, row_slack
 *      (4+nb) x 1, row_sign (4+nb) x 1 (nx = 2 dim, nu = dim; cmpc_mpc_weights); optional tol, max_iter, fp32
 *      (CMPC_FLAG_FP32), flags (further CMPC_FLAG_* bits, passed to the solver unchanged).
 *   D: struct, MATLAB order (B agents, last dimension): A nx x nx x N x B, B nu x nx x N x B, x0 nx x B,
 *      u_prev nu x B, lane 1 x B.  This is the C ABI's row-major layout read backwards, so nothing is
 *      transposed: A(j, i, k, b) is entry (i, j) of agent b's A_k.  z is nz x B, nz = (nx+3)(N+1) + 2 nu N.
 *   S: struct — nbr nb x B (0-based global agent indices; omitted: no neighbours), traj 2 x (N+1) x n_total
 *      (the initial exchange buffer), optional n_total (default B), self_offset, host_exchange, reselect
 *      (CMPC_ROUNDS_RESELECT), lpt (CMPC_ROUNDS_LPT), history (default 1).
 *
 * Handles are small integers (index into this gateway's table).  Errors through mexErrMsgIdAndTxt:
 * cmpc:di:args, cmpc:device, cmpc:solve.
 * Build in MATLAB:  mex -largeArrayDims cmpc_di_mex.c -I<repo>/include -L<repo>/colaborativempc-_amd/lib -lcmpc
 * CI builds it against the mock mex.h of tests/mex_mock.
 */
#include <string.h>

#include "cmpc.h"
#include "mex.h"

#define CMPC_MEX_FAMILY cmpc_di
#define CMPC_MEX_ARGS "cmpc:di:args"
#include "cmpc_mex_rounds.h"

/* n x n, MATLAB column-major -> row-major */
static void square(const mxArray* P, const char* name, int n, double* out) {
    const double* m = mxGetPr(field(P, name, (size_t)n * n, 1));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) out[i * n + j] = m[j * n + i];
}

static void rounds_create(mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 4) ARGS_ERROR("usage: h = cmpc_di('rounds_create', P, D, S)");
    const mxArray* P = require_struct(prhs[1], "P");
    const mxArray* D = require_struct(prhs[2], "D");
    const mxArray* S = require_struct(prhs[3], "S");
    cmpc_di_params prm;
    memset(&prm, 0, sizeof prm);
    prm.dim = (int)scalar(P, "dim");
    if (prm.dim != 2 && prm.dim != 3) ARGS_ERROR("P.dim must be 2 or 3");
    prm.v_ref = scalar(P, "v_ref"); prm.q_v = scalar(P, "q_v"); prm.q_lane = scalar(P, "q_lane");
    prm.hw = scalar(P, "hw"); prm.min_vel = scalar(P, "min_vel"); prm.max_vel = scalar(P, "max_vel");
    prm.min_dist = scalar(P, "min_dist"); prm.wq = scalar(P, "wq");
    const int N = (int)scalar(P, "N");
    if (N < 1) ARGS_ERROR("P.N must be >= 1");
    const int nx = 2 * prm.dim, nu = prm.dim;

    const mxArray* x0 = field(D, "x0", 0, 1);
    const size_t B = mxGetNumberOfElements(x0) / (size_t)nx;
    if (B * nx != mxGetNumberOfElements(x0) || B == 0) ARGS_ERROR("x0 must be nx x B");
    const mxArray* A = field(D, "A", (size_t)nx * nx * N * B, 1);
    const mxArray* Bm = field(D, "B", (size_t)nu * nx * N * B, 1);
    const mxArray* up = field(D, "u_prev", (size_t)nu * B, 1);
    const mxArray* lane = field(D, "lane", B, 1);

    const int n_total = (int)scalar_or(S, "n_total", (double)B);
    const int self_offset = (int)scalar_or(S, "self_offset", 0.0);
    if (n_total < 1) ARGS_ERROR("S.n_total must be >= 1");
    const mxArray* nbr = field(S, "nbr", 0, 0);
    const int nb = nbr ? (int)(mxGetNumberOfElements(nbr) / B) : 0;
    if (nbr && (size_t)nb * B != mxGetNumberOfElements(nbr)) ARGS_ERROR("nbr must be nb x B");
    if (4 + nb > CMPC_MAX_MC) ARGS_ERROR("at most %d neighbours per agent", CMPC_MAX_MC - 4);
    const mxArray* traj = field(S, "traj", 2 * (size_t)(N + 1) * n_total, 1);
    const int mc = 4 + nb;

    double Q[CMPC_MAX_NX * CMPC_MAX_NX], R[CMPC_MAX_NU * CMPC_MAX_NU], dR[CMPC_MAX_NU * CMPC_MAX_NU];
    int row_slack[CMPC_MAX_MC], row_sign[CMPC_MAX_MC];
    square(P, "Q", nx, Q);
    square(P, "R", nu, R);
    square(P, "dR", nu, dR);
    const double* rs = mxGetPr(field(P, "row_slack", mc, 1));
    const double* rg = mxGetPr(field(P, "row_sign", mc, 1));
    for (int r = 0; r < mc; ++r) {
        row_slack[r] = (int)rs[r];
        row_sign[r] = (int)rg[r];
    }
    const cmpc_mpc_weights w = {Q, R, dR, mxGetPr(field(P, "Qs", 3, 1)), mxGetPr(field(P, "u_ub", nu, 1)),
                                mxGetPr(field(P, "u_lb", nu, 1)), row_slack, row_sign};
    cmpc_opts opts;
    memset(&opts, 0, sizeof opts);
    opts.tol = scalar_or(P, "tol", 0.0);
    opts.max_iter = (int)scalar_or(P, "max_iter", 0.0);
    opts.flags = (int)scalar_or(P, "flags", 0.0) | (scalar_or(P, "fp32", 0.0) != 0.0 ? CMPC_FLAG_FP32 : 0);

    const int flags = (scalar_or(S, "host_exchange", 0.0) != 0.0 ? CMPC_ROUNDS_HOST_EXCHANGE : 0) |
                      (scalar_or(S, "reselect", 0.0) != 0.0 ? CMPC_ROUNDS_RESELECT : 0) |
                      (scalar_or(S, "lpt", 0.0) != 0.0 ? CMPC_ROUNDS_LPT : 0);
    const cmpc_di_rounds_dims dims = {n_total, (int)B, self_offset, N, nb, flags, (int)scalar_or(S, "history", 1.0)};
    const int slot = free_slot();
    int* inbr = nbr_ints(nbr, (size_t)nb * B);
    const cmpc_di_rounds_init init = {mxGetPr(A), mxGetPr(Bm), mxGetPr(x0), mxGetPr(up), mxGetPr(lane), inbr,
                                      mxGetPr(traj)};
    ensure_ctx();
    const int rc = cmpc_di_rounds_create(g_ctx, &prm, &w, &dims, &init, &opts, &g_tab[slot].h);
    mxFree(inbr);
    check(rc, "cmpc_di_rounds_create");
    g_tab[slot] = (rounds_slot){g_tab[slot].h, N, (int)B, nb, n_total, nx, nu, 0};
    plhs[0] = scalar_out(slot + 1);
}

static void rounds_step(mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 3) ARGS_ERROR("usage: done = cmpc_di('rounds_step', h, k)");
    int done = 0;
    check(cmpc_di_rounds_step(handle_of(prhs[1])->h, (int)mxGetScalar(prhs[2]), &done), "cmpc_di_rounds_step");
    plhs[0] = scalar_out(done);
}

static void rounds_read(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 2) ARGS_ERROR("usage: [z, status, kkt, iters, x0, u_prev, nbr] = cmpc_di('rounds_read', h)");
    const rounds_slot* t = handle_of(prhs[1]);
    const int N = t->N, B = t->B, nb = t->nb, nx = t->nx, nu = t->nu;
    const size_t nz = (size_t)(nx + 3) * (N + 1) + 2 * (size_t)nu * N;
    mxArray* Z = mxCreateDoubleMatrix(nz, B, mxREAL);
    mxArray* ST = mxCreateDoubleMatrix(1, B, mxREAL);
    mxArray* KK = mxCreateDoubleMatrix(1, B, mxREAL);
    mxArray* IT = mxCreateDoubleMatrix(1, B, mxREAL);
    mxArray* X0 = mxCreateDoubleMatrix(nx, B, mxREAL);
    mxArray* UP = mxCreateDoubleMatrix(nu, B, mxREAL);
    mxArray* NB = mxCreateDoubleMatrix(nb, B, mxREAL);
    int* iters = (int*)mxCalloc(B, sizeof(int));
    int* status = (int*)mxCalloc(B, sizeof(int));
    int* inbr = (int*)mxCalloc((size_t)(nb ? nb : 1) * B, sizeof(int));
    const cmpc_di_rounds_out o = {mxGetPr(Z), mxGetPr(KK), iters, status, mxGetPr(X0), mxGetPr(UP), nb ? inbr : NULL};
    const int rc = cmpc_di_rounds_read(t->h, &o);
    if (rc == CMPC_OK) {
        widen(IT, iters, B);
        widen(ST, status, B);
        widen(NB, inbr, (size_t)nb * B);
    }
    mxFree(iters);
    mxFree(status);
    mxFree(inbr);
    check(rc, "cmpc_di_rounds_read");
    plhs[0] = Z;
    if (nlhs > 1) plhs[1] = ST;
    if (nlhs > 2) plhs[2] = KK;
    if (nlhs > 3) plhs[3] = IT;
    if (nlhs > 4) plhs[4] = X0;
    if (nlhs > 5) plhs[5] = UP;
    if (nlhs > 6) plhs[6] = NB;
}

static void rounds_history(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 4) ARGS_ERROR("usage: [kkt, iters, status] = cmpc_di('rounds_history', h, first, count)");
    const rounds_slot* t = handle_of(prhs[1]);
    const int first = (int)mxGetScalar(prhs[2]), count = (int)mxGetScalar(prhs[3]), B = t->B;
    if (first < 0 || count < 0) ARGS_ERROR("first and count must be >= 0");
    const size_t n = (size_t)B * count;
    mxArray* KK = mxCreateDoubleMatrix(B, count, mxREAL);
    mxArray* IT = mxCreateDoubleMatrix(B, count, mxREAL);
    mxArray* ST = mxCreateDoubleMatrix(B, count, mxREAL);
    int* iters = (int*)mxCalloc(n ? n : 1, sizeof(int));
    int* status = (int*)mxCalloc(n ? n : 1, sizeof(int));
    const int rc = cmpc_di_rounds_history(t->h, first, count, mxGetPr(KK), iters, status);
    if (rc == CMPC_OK) {
        widen(IT, iters, n);
        widen(ST, status, n);
    }
    mxFree(iters);
    mxFree(status);
    check(rc, "cmpc_di_rounds_history");
    plhs[0] = KK;
    if (nlhs > 1) plhs[1] = IT;
    if (nlhs > 2) plhs[2] = ST;
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    char cmd[32];
    if (nrhs < 1 || !mxIsChar(prhs[0]) || mxGetString(prhs[0], cmd, sizeof cmd) != 0)
        ARGS_ERROR("usage: cmpc_di('rounds_create' | 'rounds_step' | 'rounds_read' | "
                   "'rounds_history' | 'rounds_log_enable' | 'rounds_log' | 'rounds_get_traj' | 'rounds_set_traj' | "
                   "'rounds_destroy' | 'comm_id' | 'comm_init', ...)");
    if (!strcmp(cmd, "rounds_create")) {
        rounds_create(plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rounds_step")) {
        rounds_step(plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rounds_read")) {
        rounds_read(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rounds_history")) {
        rounds_history(nlhs, plhs, nrhs, prhs);
    } else if (!shared_command(cmd, plhs, nrhs, prhs)) {
        ARGS_ERROR("unknown command '%s'", cmd);
    }
}
