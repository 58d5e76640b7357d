/* What the round-handle MEX gateways (cmpc_lpv_mex.c, cmpc_di_mex.c) share: the context and handle table, the
 * struct-field readers, and the commands that differ only in the family's entry points — rounds_log_enable,
 * rounds_log, rounds_get_traj / rounds_set_traj, rounds_destroy, comm_id, comm_init.
 *
 * A gateway defines, before it includes this header (after cmpc.h and mex.h),
 *   CMPC_MEX_FAMILY   cmpc_lpv | cmpc_di: the entry points <family>_rounds_*, the command name of the usage texts
 *   CMPC_MEX_ARGS     its argument-error identifier ("cmpc:lpv:args")
 * Everything here is static: a gateway stays one translation unit, built by the one `mex` line of its header.
 */
#ifndef CMPC_MEX_ROUNDS_H
#define CMPC_MEX_ROUNDS_H

#include <string.h>

#define CMPC_CAT_(a, b) a##b
#define CMPC_CAT(a, b) CMPC_CAT_(a, b)
#define CMPC_STR_(a) #a
#define CMPC_STR(a) CMPC_STR_(a)
#define ROUNDS(fn) CMPC_CAT(CMPC_MEX_FAMILY, _rounds_##fn) /* cmpc_lpv_rounds_<fn> */
#define ROUNDS_NAME(fn) CMPC_STR(ROUNDS(fn))               /* ... as a string, for check() */
#define GATEWAY CMPC_STR(CMPC_MEX_FAMILY)                  /* "cmpc_lpv" */
#define ARGS_ERROR(...) mexErrMsgIdAndTxt(CMPC_MEX_ARGS, __VA_ARGS__)

#define MAX_HANDLES 64

typedef struct {
    CMPC_CAT(CMPC_MEX_FAMILY, _rounds) * h;
    int N, B, nb, T; /* horizon, this rank's agents, neighbours per agent, n_total */
    int nx, nu;      /* state and input widths (the log's rows, rounds_read) */
    int log;         /* CMPC_LOG_* flags of rounds_log_enable */
} rounds_slot;

static cmpc_ctx* g_ctx = NULL;
static rounds_slot g_tab[MAX_HANDLES];

static void cleanup(void) {
    for (int i = 0; i < MAX_HANDLES; ++i)
        if (g_tab[i].h) {
            ROUNDS(destroy)(g_tab[i].h);
            g_tab[i].h = NULL;
        }
    if (g_ctx) cmpc_destroy(g_ctx);
    g_ctx = NULL;
}

static void ensure_ctx(void) {
    if (!g_ctx) {
        if (cmpc_create(&g_ctx, 0) != CMPC_OK) {
            g_ctx = NULL;
            mexErrMsgIdAndTxt("cmpc:device", GATEWAY ": no usable MI355X (gfx950) device");
        }
        mexAtExit(cleanup);
    }
}

static void check(int rc, const char* what) {
    if (rc != CMPC_OK) mexErrMsgIdAndTxt("cmpc:solve", "%s failed (%d): %s", what, rc, cmpc_last_error(g_ctx));
}

static const mxArray* field(const mxArray* S, const char* name, size_t numel, int required) {
    const mxArray* v = mxGetField(S, 0, name);
    if (!v || mxIsEmpty(v)) {
        if (required) ARGS_ERROR("field %s is required", name);
        return NULL;
    }
    if (!mxIsDouble(v) || mxIsComplex(v) || mxIsSparse(v)) ARGS_ERROR("field %s must be a full real double array", name);
    if (numel && mxGetNumberOfElements(v) != numel)
        ARGS_ERROR("field %s has %zu elements, expected %zu", name, mxGetNumberOfElements(v), numel);
    return v;
}

static double scalar(const mxArray* S, const char* name) { return mxGetScalar(field(S, name, 1, 1)); }

static double scalar_or(const mxArray* S, const char* name, double dflt) {
    const mxArray* v = field(S, name, 1, 0);
    return v ? mxGetScalar(v) : dflt;
}

static const mxArray* require_struct(const mxArray* a, const char* what) {
    if (!a || !mxIsStruct(a)) ARGS_ERROR("%s must be a struct", what);
    return a;
}

static mxArray* dmat3(size_t a, size_t b, size_t c) {
    mwSize d[3] = {(mwSize)a, (mwSize)b, (mwSize)c};
    return mxCreateNumericArray(3, d, mxDOUBLE_CLASS, mxREAL);
}

static mxArray* scalar_out(double v) {
    mxArray* a = mxCreateDoubleMatrix(1, 1, mxREAL);
    mxGetPr(a)[0] = v;
    return a;
}

static void widen(mxArray* dst, const int* src, size_t n) {
    for (size_t i = 0; i < n; ++i) mxGetPr(dst)[i] = src[i];
}

/* S.nbr (nb x B doubles, may be NULL) as the ABI's ints; mxFree it after create */
static int* nbr_ints(const mxArray* nbr, size_t n) {
    int* out = (int*)mxCalloc(n ? n : 1, sizeof(int));
    for (size_t i = 0; nbr && i < n; ++i) out[i] = (int)mxGetPr(nbr)[i];
    return out;
}

static int free_slot(void) {
    for (int i = 0; i < MAX_HANDLES; ++i)
        if (!g_tab[i].h) return i;
    ARGS_ERROR("too many open rounds handles (%d)", MAX_HANDLES);
    return -1;
}

static rounds_slot* handle_of(const mxArray* a) {
    if (!a || !mxIsDouble(a) || mxGetNumberOfElements(a) != 1) ARGS_ERROR("bad rounds handle");
    const int h = (int)mxGetScalar(a) - 1;
    if (h < 0 || h >= MAX_HANDLES || !g_tab[h].h) ARGS_ERROR("bad rounds handle");
    return &g_tab[h];
}

static void rounds_log_enable(int nrhs, const mxArray* prhs[]) {
    if (nrhs != 3 && nrhs != 4) ARGS_ERROR("usage: " GATEWAY "('rounds_log_enable', h, capacity [, flags])");
    rounds_slot* t = handle_of(prhs[1]);
    const int flags = nrhs > 3 ? (int)mxGetScalar(prhs[3]) : 0;
    check(ROUNDS(log_enable)(t->h, (int)mxGetScalar(prhs[2]), flags), ROUNDS_NAME(log_enable));
    t->log = flags;
}

static void rounds_log(mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 2 && nrhs != 4) ARGS_ERROR("usage: L = " GATEWAY "('rounds_log', h [, first, count])");
    const rounds_slot* t = handle_of(prhs[1]);
    const int B = t->B, sep = t->log & CMPC_LOG_SEPARATION;
    int first = 0, count = 0;
    if (nrhs == 2) {
        check(ROUNDS(log_range)(t->h, &first, &count), ROUNDS_NAME(log_range));
    } else {
        first = (int)mxGetScalar(prhs[2]);
        count = (int)mxGetScalar(prhs[3]);
    }
    if (first < 0 || count < 0) ARGS_ERROR("first and count must be >= 0");
    const size_t n = (size_t)B * count;
    mxArray* XS = dmat3(t->nx, B, count);
    mxArray* US = dmat3(t->nu, B, count);
    mxArray* LA = mxCreateDoubleMatrix(B, count, mxREAL);
    mxArray* KK = mxCreateDoubleMatrix(B, count, mxREAL);
    mxArray* IT = mxCreateDoubleMatrix(B, count, mxREAL);
    mxArray* ST = mxCreateDoubleMatrix(B, count, mxREAL);
    mxArray* S2 = mxCreateDoubleMatrix(B, count, mxREAL);
    mxArray* NR = mxCreateDoubleMatrix(B, count, mxREAL);
    mxArray* MS = mxCreateDoubleMatrix(count, 1, mxREAL);
    int* ibuf = (int*)mxCalloc(3 * (n ? n : 1), sizeof(int));
    int *iters = ibuf, *status = ibuf + (n ? n : 1), *nearest = status + (n ? n : 1);
    const cmpc_rounds_log o = {mxGetPr(XS), mxGetPr(US), mxGetPr(LA), mxGetPr(KK), iters, status,
                               sep ? mxGetPr(S2) : NULL, sep ? nearest : NULL, mxGetPr(MS)};
    const int rc = ROUNDS(log_read)(t->h, first, count, &o);
    if (rc == CMPC_OK) {
        widen(IT, iters, n);
        widen(ST, status, n);
        if (sep) widen(NR, nearest, n);
    }
    mxFree(ibuf);
    check(rc, ROUNDS_NAME(log_read));
    const char* names[] = {"first", "state", "u", "look_ahead", "kkt", "iters", "status", "solve_ms", "sep2", "nearest"};
    mxArray* L = mxCreateStructMatrix(1, 1, sep ? 10 : 8, names);
    mxArray* vals[] = {scalar_out(first), XS, US, LA, KK, IT, ST, MS, S2, NR};
    for (int i = 0; i < (sep ? 10 : 8); ++i) mxSetField(L, 0, names[i], vals[i]);
    plhs[0] = L;
}

static void rounds_traj(mxArray* plhs[], int nrhs, const mxArray* prhs[], int set) {
    if (nrhs != (set ? 3 : 2)) ARGS_ERROR("usage: rounds_get_traj(h) / rounds_set_traj(h, T)");
    const rounds_slot* t = handle_of(prhs[1]);
    if (set) {
        const mxArray* T = prhs[2];
        if (!mxIsDouble(T) || mxGetNumberOfElements(T) != 2 * (size_t)(t->N + 1) * t->T)
            ARGS_ERROR("T must be 2 x (N+1) x n_total");
        check(ROUNDS(set_traj)(t->h, mxGetPr(T)), ROUNDS_NAME(set_traj));
        return;
    }
    mxArray* T = dmat3(2, t->N + 1, t->B);
    check(ROUNDS(get_traj)(t->h, mxGetPr(T)), ROUNDS_NAME(get_traj));
    plhs[0] = T;
}

static void rounds_destroy(int nrhs, const mxArray* prhs[]) {
    if (nrhs != 2) ARGS_ERROR("usage: " GATEWAY "('rounds_destroy', h)");
    rounds_slot* t = handle_of(prhs[1]);
    ROUNDS(destroy)(t->h);
    t->h = NULL;
}

static void comm_id(mxArray* plhs[]) {
    unsigned char id[CMPC_COMM_ID_BYTES];
    if (cmpc_comm_id(id) != CMPC_OK) mexErrMsgIdAndTxt("cmpc:device", "cmpc_comm_id failed");
    plhs[0] = mxCreateDoubleMatrix(1, CMPC_COMM_ID_BYTES, mxREAL);
    for (int i = 0; i < CMPC_COMM_ID_BYTES; ++i) mxGetPr(plhs[0])[i] = id[i];
}

static void comm_init(int nrhs, const mxArray* prhs[]) {
    if (nrhs != 4 || mxGetNumberOfElements(prhs[3]) != CMPC_COMM_ID_BYTES)
        ARGS_ERROR("usage: " GATEWAY "('comm_init', nranks, rank, id)");
    unsigned char id[CMPC_COMM_ID_BYTES];
    for (int i = 0; i < CMPC_COMM_ID_BYTES; ++i) id[i] = (unsigned char)mxGetPr(prhs[3])[i];
    ensure_ctx();
    check(cmpc_comm_init(g_ctx, (int)mxGetScalar(prhs[1]), (int)mxGetScalar(prhs[2]), id), "cmpc_comm_init");
}

/* the commands both gateways have; 0: `cmd` is not one of them */
static int shared_command(const char* cmd, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (!strcmp(cmd, "rounds_log_enable")) {
        rounds_log_enable(nrhs, prhs);
    } else if (!strcmp(cmd, "rounds_log")) {
        rounds_log(plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rounds_get_traj") || !strcmp(cmd, "rounds_set_traj")) {
        rounds_traj(plhs, nrhs, prhs, cmd[7] == 's');
    } else if (!strcmp(cmd, "rounds_destroy")) {
        rounds_destroy(nrhs, prhs);
    } else if (!strcmp(cmd, "comm_id")) {
        comm_id(plhs);
    } else if (!strcmp(cmd, "comm_init")) {
        comm_init(nrhs, prhs);
    } else {
        return 0;
    }
    return 1;
}

#endif
