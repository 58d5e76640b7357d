/* cmpc_lpv — MATLAB MEX gateway over libcmpc's reference-semantics LPV path (include/cmpc.h).
 *
 * The MATLAB host of north_star drives the reference's agent model (PlannerLPV,
 * planner/lib/plan_lib/distributedPlanner/LPV_Planner.py:115-182) and its consensus loop
 * (planner/scripts/LPV_HP_N_main.py:96-117; one process per agent over ROS in
 * ROS/src/planner_experiments/src/LPV_ROS_main.py:66-77,124-150) through these calls:
 *
 *   [z, status, kkt, iters, planes] = cmpc_lpv('solve', P, D)
 *       one control step of every agent in D (cmpc_solve_lpv_batch): LPV scheduling, planes,
 *       weights, QP build and solve on the GPU.
 *   h = cmpc_lpv('rounds_create', P, D, S)           cmpc_lpv_rounds_create: device-resident rounds
 *   [done, infeasible] = cmpc_lpv('rounds_step', h, k)   k rounds (gather, solve, advance, exchange)
 *   [z, status, kkt, iters, x0, planes] = cmpc_lpv('rounds_read', h)
 *   cmpc_lpv('rounds_log_enable', h, capacity [, flags])   cmpc_lpv_rounds_log_enable: a device log of the last
 *       `capacity` rounds from here on (the rows of the reference's csv/<id>/ files); flags 1 = CMPC_LOG_SEPARATION
 *   L = cmpc_lpv('rounds_log', h [, first, count])   cmpc_lpv_rounds_log_read: rounds first .. first+count-1 (0-based,
 *       counted from create; default: all the ring holds) as a struct — first (scalar), state 9 x B x count
 *       (xPred[0]: states.dat), u 2 x B x count (uPred[0]: u.dat), look_ahead B x count (xPred[-1, 6] - xPred[0, 6]:
 *       plan_dist.dat), kkt, iters, status B x count, solve_ms count x 1 (the whole batch's solver launch in ms, the
 *       same for every agent; / 1e3 for time.dat), and with CMPC_LOG_SEPARATION sep2, nearest B x count (0-based
 *       global index of the nearest other agent)
 *   T = cmpc_lpv('rounds_get_traj', h)               this rank's predicted X, Y (host exchange)
 *   cmpc_lpv('rounds_set_traj', h, T)                the gathered exchange buffer (host exchange)
 *   cmpc_lpv('rounds_destroy', h)
 *   id = cmpc_lpv('comm_id');  cmpc_lpv('comm_init', nranks, rank, id)   RCCL exchange (one GPU per rank)
 *
 *   P: struct — model lf lr m I Cf Cr mu (config/base_class.py:20-28), limits vx_ref min_dist max_vel
 *      min_vel max_rs max_ls max_ac max_dc (:30-41), dt, wq, Q 9x9, Qs 3x1 (diagonal), R 2x2, dR 2x2
 *      (scripts/config_files/config_LPV.py:6-11), N, track (struct s0, len, curv, half_width: one
 *      entry per PointAndTangent row, track_initialization.py:220-300); optional tol, max_iter,
 *      rescue (default 1: CMPC_FLAG_RESCUE, as PlannerLPV), polish (default 1: CMPC_FLAG_POLISH with
 *      rescue, as PlannerLPV — OSQP's polish=True, LPV_Planner.py:233).
 *   D: struct, MATLAB order (B agents, last dimension): x0 9xB, x_last 9 x rows x B (rows N+1 at the
 *      first step, N afterwards), u_last 2xNxB, u_old 2xB, pose 2x(N+1)xB, x_agents 2 x nb x (N+1) x B
 *      (optional: none = no neighbours).  This is the C ABI's row-major layout read backwards, so
 *      nothing is transposed.  z is nz x B (nz = 12(N+1)+4N, LPV_Planner.py:164-178).
 *   S: struct — nbr nb x B (0-based global agent indices), optional n_total, self_offset, traj
 *      2 x (N+1) x n_total (the initial exchange buffer), host_exchange, halt (default 1).
 *
 * Handles are small integers (index into this gateway's table).  Errors through
 * mexErrMsgIdAndTxt: cmpc:lpv:args, cmpc:device, cmpc:solve.
 * Build in MATLAB:  mex -largeArrayDims cmpc_lpv_mex.c -I<repo>/include -L<repo>/colaborativempc-_amd/lib -lcmpc
 * CI builds it against the mock mex.h of tests/mex_mock.
 */
#include <math.h>
#include <string.h>

#include "cmpc.h"
#include "mex.h"

#define CMPC_MEX_FAMILY cmpc_lpv
#define CMPC_MEX_ARGS "cmpc:lpv:args"
#include "cmpc_mex_rounds.h"

/* P -> parameters, track, horizon, options */
typedef struct {
    cmpc_lpv_params prm;
    cmpc_track track;
    cmpc_opts opts;
    int N;
} lpv_setup;

static void read_params(const mxArray* P, lpv_setup* s) {
    require_struct(P, "P");
    memset(s, 0, sizeof(*s));
    cmpc_lpv_params* p = &s->prm;
    p->lf = scalar(P, "lf"); p->lr = scalar(P, "lr"); p->m = scalar(P, "m"); p->I = scalar(P, "I");
    p->Cf = scalar(P, "Cf"); p->Cr = scalar(P, "Cr"); p->mu = scalar(P, "mu");
    p->vx_ref = scalar(P, "vx_ref"); p->min_dist = scalar(P, "min_dist"); p->max_vel = scalar(P, "max_vel");
    p->min_vel = scalar(P, "min_vel"); p->max_rs = scalar(P, "max_rs"); p->max_ls = scalar(P, "max_ls");
    p->max_ac = scalar(P, "max_ac"); p->max_dc = scalar(P, "max_dc"); p->dt = scalar(P, "dt");
    p->wq = scalar(P, "wq");
    /* Q 9x9, R 2x2, dR 2x2: MATLAB column-major -> row-major (symmetric in practice; transposed anyway) */
    const double* Q = mxGetPr(field(P, "Q", 81, 1));
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) p->Q[i * 9 + j] = Q[j * 9 + i];
    const double* R = mxGetPr(field(P, "R", 4, 1));
    const double* dR = mxGetPr(field(P, "dR", 4, 1));
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            p->R[i * 2 + j] = R[j * 2 + i];
            p->dR[i * 2 + j] = dR[j * 2 + i];
        }
    const mxArray* qs = field(P, "Qs", 0, 1);
    const size_t nq = mxGetNumberOfElements(qs);
    if (nq == 3) {
        for (int j = 0; j < 3; ++j) p->Qs[j] = mxGetPr(qs)[j];
    } else if (nq == 9) {  /* the reference passes Qs as a 3x3 (diagonal) matrix */
        for (int j = 0; j < 3; ++j) p->Qs[j] = mxGetPr(qs)[j * 4];
    } else {
        ARGS_ERROR("Qs must be 3x1 or 3x3 (diagonal)");
    }
    s->N = (int)scalar(P, "N");
    const mxArray* T = require_struct(mxGetField(P, 0, "track"), "P.track");
    const mxArray* s0 = field(T, "s0", 0, 1);
    const size_t ns = mxGetNumberOfElements(s0);
    s->track.nseg = (int)ns;
    s->track.s0 = mxGetPr(s0);
    s->track.len = mxGetPr(field(T, "len", ns, 1));
    s->track.curv = mxGetPr(field(T, "curv", ns, 1));
    s->track.half_width = mxGetPr(field(T, "half_width", ns, 1));
    s->opts.tol = scalar_or(P, "tol", 0.0);
    s->opts.max_iter = (int)scalar_or(P, "max_iter", 0.0);
    s->opts.flags = scalar_or(P, "rescue", 1.0) != 0.0
                        ? CMPC_FLAG_RESCUE | (scalar_or(P, "polish", 1.0) != 0.0 ? CMPC_FLAG_POLISH : 0)
                        : 0;
}

/* D -> batch, neighbours, rows of x_last, data pointers (no copies: MATLAB order is the ABI's) */
typedef struct {
    int B, nb, rows;
    cmpc_lpv_data d;
} lpv_batch;

static void read_data(const mxArray* D, int N, lpv_batch* b) {
    require_struct(D, "D");
    const mxArray* x0 = field(D, "x0", 0, 1);
    const size_t B = mxGetNumberOfElements(x0) / 9;
    if (B * 9 != mxGetNumberOfElements(x0) || B == 0) ARGS_ERROR("x0 must be 9 x B");
    const mxArray* xl = field(D, "x_last", 0, 1);
    const size_t rows = mxGetNumberOfElements(xl) / (9 * B);
    if (rows * 9 * B != mxGetNumberOfElements(xl) || (rows != (size_t)N && rows != (size_t)N + 1))
        ARGS_ERROR("x_last must be 9 x (N or N+1) x B");
    const mxArray* xa = field(D, "x_agents", 0, 0);
    size_t nb = 0;
    if (xa) {
        nb = mxGetNumberOfElements(xa) / (2 * (size_t)(N + 1) * B);
        if (nb * 2 * (N + 1) * B != mxGetNumberOfElements(xa) || nb == 0)
            ARGS_ERROR("x_agents must be 2 x nb x (N+1) x B");
    }
    b->B = (int)B;
    b->nb = (int)nb;
    b->rows = (int)rows;
    b->d.x0 = mxGetPr(x0);
    b->d.x_last = mxGetPr(xl);
    b->d.u_last = mxGetPr(field(D, "u_last", 2 * (size_t)N * B, 1));
    const mxArray* uo = field(D, "u_old", 2 * B, 0);
    b->d.u_old = uo ? mxGetPr(uo) : NULL;
    b->d.x_agents = xa ? mxGetPr(xa) : NULL;
    b->d.pose = mxGetPr(field(D, "pose", 2 * (size_t)(N + 1) * B, 1));
}

static mxArray* planes_array(int N, int nb, int B) {
    mwSize d[4] = {(mwSize)(nb ? nb : 1), 3, (mwSize)N, (mwSize)B};
    return mxCreateNumericArray(4, d, mxDOUBLE_CLASS, mxREAL);
}

static void solve(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 3) ARGS_ERROR("usage: cmpc_lpv('solve', P, D)");
    lpv_setup s;
    read_params(prhs[1], &s);
    lpv_batch b;
    read_data(prhs[2], s.N, &b);
    double* zero_uo = NULL;
    if (!b.d.u_old) {  /* PlannerLPV's initial OldSteering / OldAccelera (LPV_Planner.py:86-87) */
        zero_uo = (double*)mxCalloc(2 * (size_t)b.B, sizeof(double));
        b.d.u_old = zero_uo;
    }
    const size_t nz = 12 * (size_t)(s.N + 1) + 4 * (size_t)s.N;
    mxArray* Z = mxCreateDoubleMatrix(nz, b.B, mxREAL);
    mxArray* KK = mxCreateDoubleMatrix(1, b.B, mxREAL);
    mxArray* IT = mxCreateDoubleMatrix(1, b.B, mxREAL);
    mxArray* ST = mxCreateDoubleMatrix(1, b.B, mxREAL);
    mxArray* PL = planes_array(s.N, b.nb, b.B);
    int* iters = (int*)mxCalloc(b.B, sizeof(int));
    int* status = (int*)mxCalloc(b.B, sizeof(int));
    cmpc_lpv_dims dims = {b.B, s.N, b.nb, b.rows};
    cmpc_lpv_out out = {mxGetPr(Z), b.nb ? mxGetPr(PL) : NULL, mxGetPr(KK), iters, status};
    ensure_ctx();
    const int rc = cmpc_solve_lpv_batch(g_ctx, &s.prm, &s.track, &dims, &b.d, &out, &s.opts);
    if (zero_uo) mxFree(zero_uo);
    check(rc, "cmpc_solve_lpv_batch");
    widen(IT, iters, b.B);
    widen(ST, status, b.B);
    mxFree(iters);
    mxFree(status);
    plhs[0] = Z;
    if (nlhs > 1) plhs[1] = ST;
    if (nlhs > 2) plhs[2] = KK;
    if (nlhs > 3) plhs[3] = IT;
    if (nlhs > 4) plhs[4] = PL;
}

static void rounds_create(mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 4) ARGS_ERROR("usage: h = cmpc_lpv('rounds_create', P, D, S)");
    lpv_setup s;
    read_params(prhs[1], &s);
    lpv_batch b;
    read_data(prhs[2], s.N, &b);
    if (b.rows != s.N + 1) ARGS_ERROR("rounds start from Last_xPredicted with N+1 rows");
    const mxArray* S = require_struct(prhs[3], "S");
    const int n_total = (int)scalar_or(S, "n_total", (double)b.B);
    const int self_offset = (int)scalar_or(S, "self_offset", 0.0);
    const mxArray* nbr = field(S, "nbr", 0, b.nb > 0);
    int nb = nbr ? (int)(mxGetNumberOfElements(nbr) / (size_t)b.B) : 0;
    if (nbr && (size_t)nb * b.B != mxGetNumberOfElements(nbr)) ARGS_ERROR("nbr must be nb x B");
    const mxArray* traj = field(S, "traj", 2 * (size_t)(s.N + 1) * n_total, 0);
    const int flags = (scalar_or(S, "host_exchange", 0.0) != 0.0 ? CMPC_ROUNDS_HOST_EXCHANGE : 0) |
                      (scalar_or(S, "halt", 1.0) != 0.0 ? 0 : CMPC_ROUNDS_NO_HALT);
    const int slot = free_slot();
    int* inbr = nbr_ints(nbr, (size_t)nb * b.B);
    cmpc_lpv_rounds_dims dims = {n_total, b.B, self_offset, s.N, nb, flags};
    cmpc_lpv_rounds_init init = {b.d.x0, b.d.x_last, b.d.u_last, b.d.u_old, inbr, traj ? mxGetPr(traj) : NULL};
    ensure_ctx();
    const int rc = cmpc_lpv_rounds_create(g_ctx, &s.prm, &s.track, &dims, &init, &s.opts, &g_tab[slot].h);
    mxFree(inbr);
    check(rc, "cmpc_lpv_rounds_create");
    g_tab[slot] = (rounds_slot){g_tab[slot].h, s.N, b.B, nb, n_total, 9, 2, 0};
    plhs[0] = scalar_out(slot + 1);
}

static void rounds_step(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 3) ARGS_ERROR("usage: [done, infeasible] = cmpc_lpv('rounds_step', h, k)");
    const rounds_slot* t = handle_of(prhs[1]);
    const int k = (int)mxGetScalar(prhs[2]);
    int done = 0, bad = 0;
    check(cmpc_lpv_rounds_step(t->h, k, &done, &bad), "cmpc_lpv_rounds_step");
    plhs[0] = scalar_out(done);
    if (nlhs > 1) plhs[1] = scalar_out(bad);
}

static void rounds_read(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 2) ARGS_ERROR("usage: [z, status, kkt, iters, x0, planes] = cmpc_lpv('rounds_read', h)");
    const rounds_slot* t = handle_of(prhs[1]);
    const int N = t->N, B = t->B, nb = t->nb;
    const size_t nz = 12 * (size_t)(N + 1) + 4 * (size_t)N;
    mxArray* Z = mxCreateDoubleMatrix(nz, B, mxREAL);
    mxArray* ST = mxCreateDoubleMatrix(1, B, mxREAL);
    mxArray* KK = mxCreateDoubleMatrix(1, B, mxREAL);
    mxArray* IT = mxCreateDoubleMatrix(1, B, mxREAL);
    mxArray* X0 = mxCreateDoubleMatrix(9, B, mxREAL);
    mxArray* PL = planes_array(N, nb, B);
    int* iters = (int*)mxCalloc(B, sizeof(int));
    int* status = (int*)mxCalloc(B, sizeof(int));
    cmpc_lpv_rounds_out o = {mxGetPr(Z), mxGetPr(KK), iters, status, mxGetPr(X0), nb ? mxGetPr(PL) : NULL};
    const int rc = cmpc_lpv_rounds_read(t->h, &o);
    if (rc == CMPC_OK) {
        widen(IT, iters, B);
        widen(ST, status, B);
    }
    mxFree(iters);
    mxFree(status);
    check(rc, "cmpc_lpv_rounds_read");
    plhs[0] = Z;
    if (nlhs > 1) plhs[1] = ST;
    if (nlhs > 2) plhs[2] = KK;
    if (nlhs > 3) plhs[3] = IT;
    if (nlhs > 4) plhs[4] = X0;
    if (nlhs > 5) plhs[5] = PL;
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    char cmd[32];
    if (nrhs < 1 || !mxIsChar(prhs[0]) || mxGetString(prhs[0], cmd, sizeof cmd) != 0)
        ARGS_ERROR("usage: cmpc_lpv('solve' | 'rounds_create' | 'rounds_step' | 'rounds_read' | "
                   "'rounds_log_enable' | 'rounds_log' | "
                   "'rounds_get_traj' | 'rounds_set_traj' | 'rounds_destroy' | 'comm_id' | "
                   "'comm_init', ...)");
    if (!strcmp(cmd, "solve")) {
        solve(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rounds_create")) {
        rounds_create(plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rounds_step")) {
        rounds_step(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rounds_read")) {
        rounds_read(nlhs, plhs, nrhs, prhs);
    } else if (!shared_command(cmd, plhs, nrhs, prhs)) {
        ARGS_ERROR("unknown command '%s'", cmd);
    }
}
