// Consensus rounds behind a handle (include/cmpc.h, cmpc_lpv_rounds_*): the device-resident loop of
// LPV_HP_N_main.py:96-117 for hosts that own no device memory (MATLAB through the MEX gateway, C).
// The handle owns this rank's agent state and the node-global exchange buffer in one device
// allocation; a round chains the C-ABI device entry points on the context's stream:
//   [cmpc_nbr_select_dev ->] cmpc_lpv_gather_dev -> cmpc_solve_lpv_batch_dev -> cmpc_lpv_advance_dev -> exchange
// where the exchange is a device copy (one rank), the RCCL all-gather of the context's
// communicator (cmpc_allgather_trajectories), or the host's (CMPC_ROUNDS_HOST_EXCHANGE).
// With the log on (cmpc_*_rounds_log_enable) a round ends with cmpc_round_log_dev [-> cmpc_nbr_select_dev, nb = 1]
// into the handle's log ring, and an event pair brackets its solver call.
// cmpc_di_rounds_* (further down) is the same handle for the synthetic double-integrator family.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"

// The experiment log of a handle (cmpc_*_rounds_log_*): a device ring of `capacity` rounds, round r in row
// r % capacity, and an event pair per row around the round's solver call.  A block of its own, made by
// log_enable after create and freed by destroy; both handles share it.
struct RoundLog {
    int capacity = 0, flags = 0;
    int first = 0;  // the log covers rounds [first, end): first = the handle's round count at enable
    int end = 0;
    cmpc_log_dims d{};
    cmpc_nbr_dims sel{};  // CMPC_LOG_SEPARATION: nb = 1, window (0, 0)
    char* mem = nullptr;
    double *state = nullptr, *u = nullptr, *look = nullptr, *kkt = nullptr, *sep2 = nullptr;
    int *iters = nullptr, *status = nullptr, *nearest = nullptr;
    std::vector<hipEvent_t> ev;  // 2 x capacity: [2 row] before, [2 row + 1] after the solver call
};

struct cmpc_lpv_rounds {
    cmpc_ctx* ctx = nullptr;
    cmpc_lpv_params prm{};
    double seg[4][CMPC_MAX_SEG]{};  // copy of the track table: s0, len, curv, half_width
    cmpc_track track{};
    cmpc_lpv_rounds_dims d{};
    cmpc_opts opts{};
    int last_rows = 0;              // N + 1 in the first round, N afterwards (LPV_HP_N_main.py:115)
    int rounds_done = 0;            // since create (the log's round numbers)
    RoundLog* log = nullptr;        // cmpc_lpv_rounds_log_enable
    char* mem = nullptr;
    double *x0 = nullptr, *x_last = nullptr, *u_last = nullptr, *u_old = nullptr, *traj_all = nullptr,
           *traj_local = nullptr, *pose = nullptr, *x_agents = nullptr, *z = nullptr, *planes = nullptr,
           *kkt = nullptr, *x_dense = nullptr;
    int *nbr = nullptr, *iters = nullptr, *status = nullptr, *infeasible = nullptr;
};

struct cmpc_di_rounds {
    cmpc_ctx* ctx = nullptr;
    cmpc_di_params prm{};
    cmpc_di_rounds_dims d{};  // history >= 1
    cmpc_mpc_dims md{};
    cmpc_opts opts{};
    // copy of the batch-shared weights (cmpc_mpc_weights holds host pointers)
    double Q[CMPC_MAX_NX * CMPC_MAX_NX]{}, R[CMPC_MAX_NU * CMPC_MAX_NU]{}, dR[CMPC_MAX_NU * CMPC_MAX_NU]{},
        Qs[CMPC_MAX_NS]{}, u_ub[CMPC_MAX_NU]{}, u_lb[CMPC_MAX_NU]{};
    int row_slack[CMPC_MAX_MC]{}, row_sign[CMPC_MAX_MC]{};
    cmpc_mpc_weights w{};
    int rounds_done = 0;  // since create: round r writes row r % history of kkt / iters / status
    RoundLog* log = nullptr;  // cmpc_di_rounds_log_enable
    char* mem = nullptr;
    double *A = nullptr, *B = nullptr, *x0 = nullptr, *u_prev = nullptr, *lane = nullptr, *traj_all = nullptr,
           *traj_local = nullptr, *qlin = nullptr, *C = nullptr, *h = nullptr, *z = nullptr, *kkt = nullptr;
    int *nbr = nullptr, *iters = nullptr, *status = nullptr, *order = nullptr;
};

namespace {

size_t nz_lpv(int N) { return 12 * (size_t)(N + 1) + 4 * (size_t)N; }
size_t nz_di(int nx, int nu, int N) { return (size_t)(nx + 3) * (N + 1) + 2 * (size_t)nu * N; }

void log_free(RoundLog* lg) {
    if (!lg) return;
    for (hipEvent_t e : lg->ev) (void)hipEventDestroy(e);
    (void)hipFree(lg->mem);
    delete lg;
}

// d: the handle's log dimensions; sel: its population (nb, k0, k1 are set here); stale: a sharded host-exchange
// handle, whose exchange buffer holds the other ranks' previous rows when a round ends
int log_enable(cmpc_ctx* ctx, RoundLog** out, int capacity, int flags, const cmpc_log_dims& d, cmpc_nbr_dims sel,
               bool stale, int round_now) {
    if (*out) return fail(ctx, CMPC_ERR_ARG, "the log is already enabled");
    if (capacity < 1) return fail(ctx, CMPC_ERR_ARG, "log capacity < 1");
    if (flags & ~CMPC_LOG_SEPARATION) return fail(ctx, CMPC_ERR_ARG, "unknown log flag");
    const bool sep = flags & CMPC_LOG_SEPARATION;
    if (sep && sel.n_total < 2) return fail(ctx, CMPC_ERR_ARG, "CMPC_LOG_SEPARATION needs n_total >= 2");
    if (sep && stale)
        return fail(ctx, CMPC_ERR_ARG,
                    "CMPC_LOG_SEPARATION on a sharded host-exchange handle: the other ranks' rows are stale when a "
                    "round ends");
    HIP_TRY(hipSetDevice(ctx->device));
    auto* lg = new RoundLog();
    lg->capacity = capacity;
    lg->flags = flags;
    lg->first = lg->end = round_now;
    lg->d = d;
    sel.nb = 1;
    sel.k0 = sel.k1 = 0;
    lg->sel = sel;
    const size_t rows = (size_t)capacity * d.batch;
    const size_t cnt8[] = {rows * d.nx, rows * d.nu, rows, rows, sep ? rows : 0};
    const size_t cnt4[] = {rows, rows, sep ? rows : 0};
    size_t bytes = 0;
    for (size_t c : cnt8) bytes += (8 * c + 255) & ~size_t(255);
    for (size_t c : cnt4) bytes += (4 * c + 255) & ~size_t(255);
    if (hipMalloc(&lg->mem, bytes) != hipSuccess) {
        lg->mem = nullptr;
        log_free(lg);
        return fail(ctx, CMPC_ERR_NOMEM, "device allocation of the log ring failed");
    }
    size_t off = 0;
    auto take = [&](size_t b) {
        char* p = lg->mem + off;
        off += (b + 255) & ~size_t(255);
        return p;
    };
    double** dp[] = {&lg->state, &lg->u, &lg->look, &lg->kkt, &lg->sep2};
    for (int i = 0; i < 5; ++i) *dp[i] = reinterpret_cast<double*>(take(8 * cnt8[i]));
    int** ip[] = {&lg->iters, &lg->status, &lg->nearest};
    for (int i = 0; i < 3; ++i) *ip[i] = reinterpret_cast<int*>(take(4 * cnt4[i]));
    if (!sep) {
        lg->sep2 = nullptr;
        lg->nearest = nullptr;
    }
    hipError_t e = hipMemsetAsync(lg->mem, 0, bytes, ctx->stream);
    for (int i = 0; e == hipSuccess && i < 2 * capacity; ++i) {
        hipEvent_t ev;
        if ((e = hipEventCreate(&ev)) == hipSuccess) lg->ev.push_back(ev);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        log_free(lg);
        return hip_fail(ctx, e, "log_enable");
    }
    *out = lg;
    return CMPC_OK;
}

// the event before (which = 0) / after (1) round r's solver call; nothing waits on it during the step
hipError_t log_mark(RoundLog* lg, int r, int which, hipStream_t s) {
    return lg ? hipEventRecord(lg->ev[2 * (size_t)(r % lg->capacity) + which], s) : hipSuccess;
}

// round r's solver call failed after its first event was recorded: row r % capacity no longer times round
// r - capacity, which leaves the log
void log_abandon(RoundLog* lg, int r) {
    if (lg) lg->first = std::max(lg->first, std::min(lg->end, r - lg->capacity + 1));
}

// round r's rows, stream-ordered after its exchange
int log_round(cmpc_ctx* ctx, RoundLog* lg, int r, const double* z, const double* kkt, const int* iters,
              const int* status, const double* traj_all, hipStream_t s) {
    const size_t row = (size_t)(r % lg->capacity) * lg->d.batch;
    const cmpc_log_row dst{lg->state + row * lg->d.nx, lg->u + row * lg->d.nu, lg->look + row,
                           lg->kkt + row, lg->iters + row, lg->status + row};
    int rc = cmpc_round_log_dev(ctx, &lg->d, z, kkt, iters, status, &dst, s);
    if (rc == CMPC_OK && (lg->flags & CMPC_LOG_SEPARATION))
        rc = cmpc_nbr_select_dev(ctx, &lg->sel, traj_all, lg->nearest + row, lg->sep2 + row, s);
    if (rc != CMPC_OK) return rc;
    if (r != lg->end) lg->first = r;  // a round in between went unlogged (its exchange failed): the log restarts here
    lg->end = r + 1;
    return CMPC_OK;
}

int log_range(cmpc_ctx* ctx, const RoundLog* lg, int* first_round, int* count) {
    if (!lg) return fail(ctx, CMPC_ERR_ARG, "the log is not enabled (log_enable)");
    const int lo = std::max(lg->first, lg->end - lg->capacity);
    if (first_round) *first_round = lo;
    if (count) *count = lg->end - lo;
    return CMPC_OK;
}

int log_read(cmpc_ctx* ctx, const RoundLog* lg, int first_round, int count, const cmpc_rounds_log* o) {
    if (!lg) return fail(ctx, CMPC_ERR_ARG, "the log is not enabled (log_enable)");
    if (!o) return fail(ctx, CMPC_ERR_ARG, "null output");
    if (!(lg->flags & CMPC_LOG_SEPARATION) && (o->sep2 || o->nearest))
        return fail(ctx, CMPC_ERR_ARG, "sep2 / nearest: the log was enabled without CMPC_LOG_SEPARATION");
    if (first_round < 0 || count < 0 || (long long)first_round + count > lg->end)
        return fail(ctx, CMPC_ERR_ARG, "log: a round that has not run yet");
    if (count > 0 && first_round < std::max(lg->first, lg->end - lg->capacity))
        return fail(ctx, CMPC_ERR_ARG, "log: a round from before log_enable, or one the ring has already overwritten");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the ring's rows of the range: [r0, r0 + n1), then [0, count - n1) after the wrap
    const size_t B = lg->d.batch, r0 = (size_t)(first_round % lg->capacity),
                 n1 = std::min((size_t)count, lg->capacity - r0), n2 = count - n1;
    auto pull = [&](void* dst, const void* src, size_t row_bytes) {
        if (!dst || !count || !row_bytes) return hipSuccess;
        hipError_t e = hipMemcpyAsync(dst, (const char*)src + r0 * row_bytes, n1 * row_bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && n2)
            e = hipMemcpyAsync((char*)dst + n1 * row_bytes, src, n2 * row_bytes, hipMemcpyDeviceToHost, s);
        return e;
    };
    HIP_TRY(pull(o->state, lg->state, 8 * B * lg->d.nx));
    HIP_TRY(pull(o->u, lg->u, 8 * B * lg->d.nu));
    HIP_TRY(pull(o->look_ahead, lg->look, 8 * B));
    HIP_TRY(pull(o->kkt, lg->kkt, 8 * B));
    HIP_TRY(pull(o->iters, lg->iters, 4 * B));
    HIP_TRY(pull(o->status, lg->status, 4 * B));
    HIP_TRY(pull(o->sep2, lg->sep2, 8 * B));
    HIP_TRY(pull(o->nearest, lg->nearest, 4 * B));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; o->solve_ms && i < count; ++i) {
        const size_t row = (size_t)((first_round + i) % lg->capacity);
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, lg->ev[2 * row], lg->ev[2 * row + 1]));
        o->solve_ms[i] = ms;
    }
    return CMPC_OK;
}

}  // namespace

extern "C" {

int cmpc_lpv_rounds_create(cmpc_ctx* ctx, const cmpc_lpv_params* prm, const cmpc_track* track,
                           const cmpc_lpv_rounds_dims* dims, const cmpc_lpv_rounds_init* in, const cmpc_opts* opts,
                           cmpc_lpv_rounds** out) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!out || !prm || !track || !dims || !in) return fail(ctx, CMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const cmpc_lpv_rounds_dims& d = *dims;
    if (d.N < 1 || d.nb < 0 || 4 + d.nb > CMPC_MAX_MC || d.batch < 1 || d.n_total < d.batch || d.self_offset < 0 ||
        d.self_offset + d.batch > d.n_total)
        return fail(ctx, CMPC_ERR_ARG, "bad rounds dimensions (1 <= batch, self_offset + batch <= n_total, nb <= 12)");
    if (d.flags & ~(CMPC_ROUNDS_HOST_EXCHANGE | CMPC_ROUNDS_NO_HALT | CMPC_ROUNDS_RESELECT))
        return fail(ctx, CMPC_ERR_ARG, "unknown rounds flag");
    if ((d.flags & CMPC_ROUNDS_RESELECT) && d.nb >= d.n_total)
        return fail(ctx, CMPC_ERR_ARG, "CMPC_ROUNDS_RESELECT selects nb < n_total neighbours");
    if (track->nseg < 1 || track->nseg > CMPC_MAX_SEG) return fail(ctx, CMPC_ERR_UNSUPPORTED, "track has 1..32 segments");
    if (!in->x0 || !in->x_last || !in->u_last || (d.nb > 0 && !in->nbr))
        return fail(ctx, CMPC_ERR_ARG, "null initial state");
    if (!in->traj && d.batch != d.n_total)
        return fail(ctx, CMPC_ERR_ARG, "a sharded population needs the initial exchange buffer (init->traj)");
    if (d.batch != d.n_total && !(d.flags & CMPC_ROUNDS_HOST_EXCHANGE) &&
        (!ctx->comm || (long)ctx->nranks * d.batch != d.n_total || ctx->rank * d.batch != d.self_offset))
        return fail(ctx, CMPC_ERR_ARG,
                    "a sharded population exchanges over the context's communicator (cmpc_comm_init: equal "
                    "contiguous shards in rank order) or the host's (CMPC_ROUNDS_HOST_EXCHANGE)");
    for (int i = 0; in->nbr && i < d.batch * d.nb; ++i)
        if (in->nbr[i] < 0 || in->nbr[i] >= d.n_total) return fail(ctx, CMPC_ERR_ARG, "neighbour index out of range");
    if (opts && (opts->flags & ~CMPC_FLAG_ALL)) return fail(ctx, CMPC_ERR_ARG, "unknown option flag");
    HIP_TRY(hipSetDevice(ctx->device));

    auto* h = new cmpc_lpv_rounds();
    h->ctx = ctx;
    h->prm = *prm;
    h->d = d;
    if (opts) h->opts = *opts;
    h->opts.stamps = nullptr;
    h->opts.order = nullptr;
    h->last_rows = d.N + 1;
    const int ns = track->nseg;
    std::memcpy(h->seg[0], track->s0, sizeof(double) * ns);
    std::memcpy(h->seg[1], track->len, sizeof(double) * ns);
    std::memcpy(h->seg[2], track->curv, sizeof(double) * ns);
    std::memcpy(h->seg[3], track->half_width, sizeof(double) * ns);
    h->track = cmpc_track{ns, h->seg[0], h->seg[1], h->seg[2], h->seg[3]};

    const size_t B = d.batch, N = d.N, nb = d.nb, T = d.n_total, row = (N + 1) * 2;
    const size_t cnt[] = {B * 9, B * (N + 1) * 9, B * N * 2, B * 2, T * row, B * row, B * row,
                          B * row * (nb ? nb : 1), B * nz_lpv(d.N), B * N * 3 * (nb ? nb : 1), B, B * N * 9};
    size_t bytes = 0;
    for (size_t c : cnt) bytes += ((8 * c + 255) & ~size_t(255));
    bytes += 4 * ((B * (nb ? nb : 1) + 63) & ~size_t(63)) + 3 * 4 * ((B + 63) & ~size_t(63)) + 256;
    if (hipMalloc(&h->mem, bytes) != hipSuccess) {
        delete h;
        return fail(ctx, CMPC_ERR_NOMEM, "device allocation of the rounds state failed");
    }
    size_t off = 0;
    auto take = [&](size_t b) {
        char* p = h->mem + off;
        off += (b + 255) & ~size_t(255);
        return p;
    };
    double** dp[] = {&h->x0, &h->x_last, &h->u_last, &h->u_old, &h->traj_all, &h->traj_local, &h->pose,
                     &h->x_agents, &h->z, &h->planes, &h->kkt, &h->x_dense};
    for (int i = 0; i < 12; ++i) *dp[i] = reinterpret_cast<double*>(take(8 * cnt[i]));
    h->nbr = reinterpret_cast<int*>(take(4 * B * (nb ? nb : 1)));
    h->iters = reinterpret_cast<int*>(take(4 * B));
    h->status = reinterpret_cast<int*>(take(4 * B));
    h->infeasible = reinterpret_cast<int*>(take(4 * B));

    hipStream_t s = ctx->stream;
    auto up = [&](void* dst, const void* src, size_t b) { return hipMemcpyAsync(dst, src, b, hipMemcpyHostToDevice, s); };
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = up(h->x0, in->x0, 8 * B * 9);
    if (e == hipSuccess) e = up(h->x_last, in->x_last, 8 * B * (N + 1) * 9);
    if (e == hipSuccess) e = up(h->u_last, in->u_last, 8 * B * N * 2);
    if (e == hipSuccess) e = in->u_old ? up(h->u_old, in->u_old, 8 * B * 2) : hipMemsetAsync(h->u_old, 0, 8 * B * 2, s);
    if (e == hipSuccess && nb) e = up(h->nbr, in->nbr, 4 * B * nb);
    if (e == hipSuccess) e = hipMemsetAsync(h->planes, 0, 8 * B * N * 3 * (nb ? nb : 1), s);
    if (e == hipSuccess && in->traj) e = up(h->traj_all, in->traj, 8 * T * row);
    if (e == hipSuccess && !in->traj)  // the reference's initial `agents` = the predictions' X, Y (misc.py:155-165)
        e = hipMemcpy2DAsync(h->traj_all, 16, h->x_last + 7, 72, 16, B * (N + 1), hipMemcpyDeviceToDevice, s);
    // this rank's rows of the exchange buffer: an agent that is not advanced keeps its initial ones
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->traj_local, h->traj_all + (size_t)d.self_offset * row, 8 * B * row,
                           hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(h->mem);
        delete h;
        return hip_fail(ctx, e, "cmpc_lpv_rounds_create: upload");
    }
    *out = h;
    return CMPC_OK;
}

int cmpc_lpv_rounds_step(cmpc_lpv_rounds* h, int rounds, int* rounds_done, int* infeasible) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (rounds < 0) return fail(ctx, CMPC_ERR_ARG, "negative round count");
    const bool host_x = h->d.flags & CMPC_ROUNDS_HOST_EXCHANGE, sharded = h->d.batch != h->d.n_total;
    if (host_x && sharded && rounds > 1)
        return fail(ctx, CMPC_ERR_ARG, "host exchange: one round per step (exchange between steps)");
    const bool halt = !(h->d.flags & CMPC_ROUNDS_NO_HALT);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const cmpc_di_dims rd{h->d.batch, h->d.N, h->d.nb, h->d.self_offset};
    const int nb = h->d.nb;
    const cmpc_nbr_dims sd{h->d.batch, h->d.N, nb, h->d.self_offset, h->d.n_total, 0, 0};
    int done = 0, bad = 0, rc;
    for (int r = 0; r < rounds; ++r) {
        // CMPC_ROUNDS_RESELECT: this round's neighbours are the nb nearest in the exchange buffer as it stands
        if ((h->d.flags & CMPC_ROUNDS_RESELECT) &&
            (rc = cmpc_nbr_select_dev(ctx, &sd, h->traj_all, h->nbr, nullptr, s)) != CMPC_OK)
            return rc;
        if ((rc = cmpc_lpv_gather_dev(ctx, &rd, h->nbr, h->traj_all, nb ? h->x_agents : nullptr, h->pose, s)) != CMPC_OK)
            return rc;
        const cmpc_lpv_dims ld{h->d.batch, h->d.N, nb, h->last_rows};
        const cmpc_lpv_data din{h->x0, h->x_last, h->u_last, h->u_old, nb ? h->x_agents : nullptr, h->pose};
        const cmpc_lpv_out dout{h->z, nb ? h->planes : nullptr, h->kkt, h->iters, h->status};
        HIP_TRY(log_mark(h->log, h->rounds_done, 0, s));
        if ((rc = cmpc_solve_lpv_batch_dev(ctx, &h->prm, &h->track, &ld, &din, &dout, &h->opts, s)) != CMPC_OK) {
            log_abandon(h->log, h->rounds_done);
            return rc;
        }
        HIP_TRY(log_mark(h->log, h->rounds_done, 1, s));
        HIP_TRY(hipMemsetAsync(h->infeasible, 0, sizeof(int), s));
        if (h->last_rows == h->d.N + 1) {
            // first round: Last_xPredicted goes from N + 1 rows per agent to N dense ones.  The advance
            // rewrites each agent's dense slot from its solution, but an agent it does not advance
            // (no finite solution) must find its own previous rows there, not bytes of the
            // (N + 1)-row layout: compact the layout first (rows 0..N-1 of each agent)
            const size_t w = 8 * (size_t)h->d.N * 9;
            HIP_TRY(hipMemcpy2DAsync(h->x_dense, w, h->x_last, w + 72, w, h->d.batch, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(h->x_last, h->x_dense, w * h->d.batch, hipMemcpyDeviceToDevice, s));
        }
        if ((rc = cmpc_lpv_advance_dev(ctx, &rd, h->z, h->x0, h->x_last, h->u_last, h->u_old, h->traj_local, h->status,
                                       h->infeasible, s)) != CMPC_OK)
            return rc;
        h->last_rows = h->d.N;  // x_old = xPred[1:] from now on (LPV_HP_N_main.py:115)
        const size_t row = 2 * (size_t)(h->d.N + 1);
        if (!sharded) {
            HIP_TRY(hipMemcpyAsync(h->traj_all, h->traj_local, 8 * row * h->d.batch, hipMemcpyDeviceToDevice, s));
        } else if (!host_x) {
            if ((rc = cmpc_allgather_trajectories(ctx, h->traj_local, h->traj_all, row * h->d.batch, s)) != CMPC_OK)
                return rc;
        }
        // the node's infeasible count, not this rank's: the reference's loop quits for every agent
        // at once (LPV_HP_N_main.py:102-111), so every rank must take the same halt decision (a
        // rank that broke alone would leave the others waiting in the next round's all-gather).
        // The host exchange runs one round per step: its caller combines the counts it returns.
        if (sharded && !host_x && (rc = cmpc_comm_sum_i32(ctx, h->infeasible, 1, s)) != CMPC_OK) return rc;
        // the log's rows of this round (a round that halts the loop below has run, and is logged)
        if (h->log && (rc = log_round(ctx, h->log, h->rounds_done, h->z, h->kkt, h->iters, h->status, h->traj_all,
                                      s)) != CMPC_OK)
            return rc;
        ++h->rounds_done;
        ++done;
        if (halt || r + 1 == rounds) {  // the reference stops the experiment at an infeasible agent
            HIP_TRY(hipMemcpyAsync(&bad, h->infeasible, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (halt && bad) break;
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (rounds_done) *rounds_done = done;
    if (infeasible) *infeasible = bad;
    return CMPC_OK;
}

int cmpc_lpv_rounds_read(cmpc_lpv_rounds* h, const cmpc_lpv_rounds_out* o) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!o) return fail(ctx, CMPC_ERR_ARG, "null output");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = h->d.batch;
    auto dn = [&](void* dst, const void* src, size_t b) { return hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, s); };
    if (o->z) HIP_TRY(dn(o->z, h->z, 8 * B * nz_lpv(h->d.N)));
    if (o->kkt) HIP_TRY(dn(o->kkt, h->kkt, 8 * B));
    if (o->iters) HIP_TRY(dn(o->iters, h->iters, 4 * B));
    if (o->status) HIP_TRY(dn(o->status, h->status, 4 * B));
    if (o->x0) HIP_TRY(dn(o->x0, h->x0, 8 * B * 9));
    if (o->planes && h->d.nb) HIP_TRY(dn(o->planes, h->planes, 8 * B * h->d.N * 3 * h->d.nb));
    HIP_TRY(hipStreamSynchronize(s));
    return CMPC_OK;
}

int cmpc_lpv_rounds_get_traj(cmpc_lpv_rounds* h, double* traj_local) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!traj_local) return fail(ctx, CMPC_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(traj_local, h->traj_local, 16 * (size_t)(h->d.N + 1) * h->d.batch, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CMPC_OK;
}

int cmpc_lpv_rounds_set_traj(cmpc_lpv_rounds* h, const double* traj_all) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!traj_all) return fail(ctx, CMPC_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h->traj_all, traj_all, 16 * (size_t)(h->d.N + 1) * h->d.n_total, hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CMPC_OK;
}

int cmpc_lpv_rounds_destroy(cmpc_lpv_rounds* h) {
    if (!h) return CMPC_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    log_free(h->log);
    (void)hipFree(h->mem);
    delete h;
    return CMPC_OK;
}

int cmpc_lpv_rounds_log_enable(cmpc_lpv_rounds* h, int capacity, int flags) {
    if (!h) return CMPC_ERR_ARG;
    const cmpc_lpv_rounds_dims& d = h->d;
    const cmpc_log_dims ld{d.batch, 9, 2, 3, d.N, 6};
    const cmpc_nbr_dims sd{d.batch, d.N, 1, d.self_offset, d.n_total, 0, 0};
    return log_enable(h->ctx, &h->log, capacity, flags, ld, sd,
                      (d.flags & CMPC_ROUNDS_HOST_EXCHANGE) && d.batch != d.n_total, h->rounds_done);
}

int cmpc_lpv_rounds_log_range(cmpc_lpv_rounds* h, int* first_round, int* count) {
    return h ? log_range(h->ctx, h->log, first_round, count) : CMPC_ERR_ARG;
}

int cmpc_lpv_rounds_log_read(cmpc_lpv_rounds* h, int first_round, int count, const cmpc_rounds_log* o) {
    return h ? log_read(h->ctx, h->log, first_round, count, o) : CMPC_ERR_ARG;
}

// ---- the synthetic double-integrator family (cmpc_di_rounds_*): what cmpc.rounds.DIRounds.step() chains ----
//   [cmpc_nbr_select_dev ->] cmpc_di_round_dev -> [cmpc_order_by_iters_dev ->] exchange

int cmpc_di_rounds_create(cmpc_ctx* ctx, const cmpc_di_params* prm, const cmpc_mpc_weights* w,
                          const cmpc_di_rounds_dims* dims, const cmpc_di_rounds_init* in, const cmpc_opts* opts,
                          cmpc_di_rounds** out) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!out || !prm || !w || !dims || !in) return fail(ctx, CMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const cmpc_di_rounds_dims& d = *dims;
    if (d.N < 1 || d.nb < 0 || 4 + d.nb > CMPC_MAX_MC || d.batch < 1 || d.n_total < d.batch || d.self_offset < 0 ||
        d.self_offset + d.batch > d.n_total)
        return fail(ctx, CMPC_ERR_ARG, "bad rounds dimensions (1 <= batch, self_offset + batch <= n_total, nb <= 12)");
    if (prm->dim != 2 && prm->dim != 3) return fail(ctx, CMPC_ERR_ARG, "double-integrator agents have dim 2 or 3");
    if (d.history < 0) return fail(ctx, CMPC_ERR_ARG, "negative history");
    if (d.flags & ~(CMPC_ROUNDS_HOST_EXCHANGE | CMPC_ROUNDS_NO_HALT | CMPC_ROUNDS_RESELECT | CMPC_ROUNDS_LPT))
        return fail(ctx, CMPC_ERR_ARG, "unknown rounds flag");
    if ((d.flags & CMPC_ROUNDS_RESELECT) && d.nb >= d.n_total)
        return fail(ctx, CMPC_ERR_ARG, "CMPC_ROUNDS_RESELECT selects nb < n_total neighbours");
    if (!w->Q || !w->R || !w->dR || !w->Qs || !w->u_ub || !w->u_lb || !w->row_slack || !w->row_sign)
        return fail(ctx, CMPC_ERR_ARG, "null weights");
    if (!in->A || !in->B || !in->x0 || !in->u_prev || !in->lane || !in->traj || (d.nb > 0 && !in->nbr))
        return fail(ctx, CMPC_ERR_ARG, "null initial state");
    if (d.batch != d.n_total && !(d.flags & CMPC_ROUNDS_HOST_EXCHANGE) &&
        (!ctx->comm || (long)ctx->nranks * d.batch != d.n_total || ctx->rank * d.batch != d.self_offset))
        return fail(ctx, CMPC_ERR_ARG,
                    "a sharded population exchanges over the context's communicator (cmpc_comm_init: equal "
                    "contiguous shards in rank order) or the host's (CMPC_ROUNDS_HOST_EXCHANGE)");
    for (int i = 0; in->nbr && i < d.batch * d.nb; ++i)
        if (in->nbr[i] < 0 || in->nbr[i] >= d.n_total) return fail(ctx, CMPC_ERR_ARG, "neighbour index out of range");
    if (opts && (opts->flags & ~CMPC_FLAG_ALL)) return fail(ctx, CMPC_ERR_ARG, "unknown option flag");
    HIP_TRY(hipSetDevice(ctx->device));

    auto* h = new cmpc_di_rounds();
    h->ctx = ctx;
    h->prm = *prm;
    h->d = d;
    if (h->d.history == 0) h->d.history = 1;
    if (opts) h->opts = *opts;
    h->opts.stamps = nullptr;
    h->opts.order = nullptr;
    const int nx = 2 * prm->dim, nu = prm->dim, mc = 4 + d.nb;
    h->md = cmpc_mpc_dims{nx, nu, d.N, 3, mc, d.batch};
    std::memcpy(h->Q, w->Q, sizeof(double) * nx * nx);
    std::memcpy(h->R, w->R, sizeof(double) * nu * nu);
    std::memcpy(h->dR, w->dR, sizeof(double) * nu * nu);
    std::memcpy(h->Qs, w->Qs, sizeof(double) * 3);
    std::memcpy(h->u_ub, w->u_ub, sizeof(double) * nu);
    std::memcpy(h->u_lb, w->u_lb, sizeof(double) * nu);
    std::memcpy(h->row_slack, w->row_slack, sizeof(int) * mc);
    std::memcpy(h->row_sign, w->row_sign, sizeof(int) * mc);
    h->w = cmpc_mpc_weights{h->Q, h->R, h->dR, h->Qs, h->u_ub, h->u_lb, h->row_slack, h->row_sign};

    const size_t B = d.batch, N = d.N, nb = d.nb, T = d.n_total, row = (N + 1) * 2, H = h->d.history;
    const size_t cnt[] = {B * N * nx * nx, B * N * nx * nu, B * nx, B * nu, B, T * row, B * row,
                          B * (N + 1) * nx, B * N * mc * nx, B * N * mc, B * nz_di(nx, nu, d.N), H * B};
    size_t bytes = 0;
    for (size_t c : cnt) bytes += ((8 * c + 255) & ~size_t(255));
    bytes += ((4 * B * (nb ? nb : 1) + 255) & ~size_t(255)) + 2 * ((4 * H * B + 255) & ~size_t(255)) +
             ((4 * B + 255) & ~size_t(255));
    if (hipMalloc(&h->mem, bytes) != hipSuccess) {
        delete h;
        return fail(ctx, CMPC_ERR_NOMEM, "device allocation of the rounds state failed");
    }
    size_t off = 0;
    auto take = [&](size_t b) {
        char* p = h->mem + off;
        off += (b + 255) & ~size_t(255);
        return p;
    };
    double** dp[] = {&h->A, &h->B, &h->x0, &h->u_prev, &h->lane, &h->traj_all, &h->traj_local, &h->qlin, &h->C,
                     &h->h, &h->z, &h->kkt};
    for (int i = 0; i < 12; ++i) *dp[i] = reinterpret_cast<double*>(take(8 * cnt[i]));
    h->nbr = reinterpret_cast<int*>(take(4 * B * (nb ? nb : 1)));
    h->iters = reinterpret_cast<int*>(take(4 * H * B));
    h->status = reinterpret_cast<int*>(take(4 * H * B));
    h->order = reinterpret_cast<int*>(take(4 * B));

    hipStream_t s = ctx->stream;
    auto up = [&](void* dst, const void* src, size_t b) { return hipMemcpyAsync(dst, src, b, hipMemcpyHostToDevice, s); };
    hipError_t e = hipMemsetAsync(h->mem, 0, bytes, s);  // a read before the first round returns zeros
    if (e == hipSuccess) e = up(h->A, in->A, 8 * cnt[0]);
    if (e == hipSuccess) e = up(h->B, in->B, 8 * cnt[1]);
    if (e == hipSuccess) e = up(h->x0, in->x0, 8 * cnt[2]);
    if (e == hipSuccess) e = up(h->u_prev, in->u_prev, 8 * cnt[3]);
    if (e == hipSuccess) e = up(h->lane, in->lane, 8 * cnt[4]);
    if (e == hipSuccess) e = up(h->traj_all, in->traj, 8 * cnt[5]);
    if (e == hipSuccess && nb) e = up(h->nbr, in->nbr, 4 * B * nb);
    // this rank's rows of the exchange buffer until the first round writes them
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->traj_local, h->traj_all + (size_t)d.self_offset * row, 8 * B * row,
                           hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(h->mem);
        delete h;
        return hip_fail(ctx, e, "cmpc_di_rounds_create: upload");
    }
    *out = h;
    return CMPC_OK;
}

int cmpc_di_rounds_step(cmpc_di_rounds* h, int rounds, int* rounds_done) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (rounds_done) *rounds_done = 0;
    if (rounds < 0) return fail(ctx, CMPC_ERR_ARG, "negative round count");
    const bool host_x = h->d.flags & CMPC_ROUNDS_HOST_EXCHANGE, sharded = h->d.batch != h->d.n_total;
    if (host_x && sharded && rounds > 1)
        return fail(ctx, CMPC_ERR_ARG, "host exchange: one round per step (exchange between steps)");
    const bool lpt = h->d.flags & CMPC_ROUNDS_LPT;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = h->d.batch, row = 2 * (size_t)(h->d.N + 1);
    const cmpc_di_dims rd{h->d.batch, h->d.N, h->d.nb, h->d.self_offset};
    const cmpc_nbr_dims sd{h->d.batch, h->d.N, h->d.nb, h->d.self_offset, h->d.n_total, 0, 0};
    const cmpc_mpc_data din{h->A, h->B, h->x0, h->u_prev, h->qlin, h->C, h->h};
    int done = 0, rc = CMPC_OK;
    for (int r = 0; r < rounds && rc == CMPC_OK; ++r) {
        const size_t slot = (size_t)(h->rounds_done % h->d.history) * B;  // this round's row of the history ring
        const cmpc_mpc_out dout{h->z, h->kkt + slot, h->iters + slot, h->status + slot};
        if ((h->d.flags & CMPC_ROUNDS_RESELECT) && h->d.nb > 0 &&
            (rc = cmpc_nbr_select_dev(ctx, &sd, h->traj_all, h->nbr, nullptr, s)) != CMPC_OK)
            break;
        h->opts.order = (lpt && h->rounds_done > 0) ? h->order : nullptr;
        hipError_t ev = log_mark(h->log, h->rounds_done, 0, s);
        if (ev != hipSuccess) {
            rc = hip_fail(ctx, ev, "cmpc_di_rounds_step: log event");
            break;
        }
        if ((rc = cmpc_di_round_dev(ctx, &h->prm, &rd, h->nbr, h->lane, h->traj_all, &h->md, &h->w, &din, &dout,
                                    &h->opts, h->traj_local, s)) != CMPC_OK) {
            log_abandon(h->log, h->rounds_done);
            break;
        }
        if ((ev = log_mark(h->log, h->rounds_done, 1, s)) != hipSuccess) {
            rc = hip_fail(ctx, ev, "cmpc_di_rounds_step: log event");
            break;
        }
        // the next round's launch order, stream-ordered after this solve
        if (lpt && (rc = cmpc_order_by_iters_dev(ctx, h->d.batch, h->iters + slot, h->order, s)) != CMPC_OK) break;
        ++h->rounds_done;  // the round's outputs exist from here on, whatever the exchange returns
        ++done;
        if (!sharded) {
            hipError_t e = hipMemcpyAsync(h->traj_all, h->traj_local, 8 * row * B, hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) rc = hip_fail(ctx, e, "cmpc_di_rounds_step: exchange");
        } else if (!host_x) {
            rc = cmpc_allgather_trajectories(ctx, h->traj_local, h->traj_all, row * B, s);
        }
        // the log's rows of this round, from the history-ring row the solver wrote
        if (h->log && rc == CMPC_OK)
            rc = log_round(ctx, h->log, h->rounds_done - 1, h->z, h->kkt + slot, h->iters + slot, h->status + slot,
                           h->traj_all, s);
    }
    // one host synchronisation, also after an error: the rounds already queued have then finished
    const hipError_t e = hipStreamSynchronize(s);
    if (rounds_done) *rounds_done = done;
    if (rc != CMPC_OK) return rc;
    HIP_TRY(e);
    return CMPC_OK;
}

int cmpc_di_rounds_read(cmpc_di_rounds* h, const cmpc_di_rounds_out* o) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!o) return fail(ctx, CMPC_ERR_ARG, "null output");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = h->d.batch;
    const size_t slot = (size_t)((h->rounds_done > 0 ? h->rounds_done - 1 : 0) % h->d.history) * B;
    auto dn = [&](void* dst, const void* src, size_t b) { return hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, s); };
    if (o->z) HIP_TRY(dn(o->z, h->z, 8 * B * nz_di(h->md.nx, h->md.nu, h->d.N)));
    if (o->kkt) HIP_TRY(dn(o->kkt, h->kkt + slot, 8 * B));
    if (o->iters) HIP_TRY(dn(o->iters, h->iters + slot, 4 * B));
    if (o->status) HIP_TRY(dn(o->status, h->status + slot, 4 * B));
    if (o->x0) HIP_TRY(dn(o->x0, h->x0, 8 * B * h->md.nx));
    if (o->u_prev) HIP_TRY(dn(o->u_prev, h->u_prev, 8 * B * h->md.nu));
    if (o->nbr && h->d.nb) HIP_TRY(dn(o->nbr, h->nbr, 4 * B * h->d.nb));
    HIP_TRY(hipStreamSynchronize(s));
    return CMPC_OK;
}

int cmpc_di_rounds_history(cmpc_di_rounds* h, int first_round, int count, double* kkt, int* iters, int* status) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (first_round < 0 || count < 0 || (long long)first_round + count > h->rounds_done)
        return fail(ctx, CMPC_ERR_ARG, "history: a round that has not run yet");
    if (count > 0 && first_round < h->rounds_done - h->d.history)
        return fail(ctx, CMPC_ERR_ARG, "history: a round the ring has already overwritten (dims.history rounds are kept)");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = h->d.batch;
    for (int i = 0; i < count; ++i) {
        const size_t slot = (size_t)((first_round + i) % h->d.history) * B;
        if (kkt) HIP_TRY(hipMemcpyAsync(kkt + i * B, h->kkt + slot, 8 * B, hipMemcpyDeviceToHost, s));
        if (iters) HIP_TRY(hipMemcpyAsync(iters + i * B, h->iters + slot, 4 * B, hipMemcpyDeviceToHost, s));
        if (status) HIP_TRY(hipMemcpyAsync(status + i * B, h->status + slot, 4 * B, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return CMPC_OK;
}

int cmpc_di_rounds_get_traj(cmpc_di_rounds* h, double* traj_local) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!traj_local) return fail(ctx, CMPC_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(traj_local, h->traj_local, 16 * (size_t)(h->d.N + 1) * h->d.batch, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CMPC_OK;
}

int cmpc_di_rounds_set_traj(cmpc_di_rounds* h, const double* traj_all) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!traj_all) return fail(ctx, CMPC_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h->traj_all, traj_all, 16 * (size_t)(h->d.N + 1) * h->d.n_total, hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CMPC_OK;
}

int cmpc_di_rounds_destroy(cmpc_di_rounds* h) {
    if (!h) return CMPC_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    log_free(h->log);
    (void)hipFree(h->mem);
    delete h;
    return CMPC_OK;
}

int cmpc_di_rounds_log_enable(cmpc_di_rounds* h, int capacity, int flags) {
    if (!h) return CMPC_ERR_ARG;
    const cmpc_di_rounds_dims& d = h->d;
    const cmpc_log_dims ld{d.batch, h->md.nx, h->md.nu, 3, d.N, 0};
    const cmpc_nbr_dims sd{d.batch, d.N, 1, d.self_offset, d.n_total, 0, 0};
    return log_enable(h->ctx, &h->log, capacity, flags, ld, sd,
                      (d.flags & CMPC_ROUNDS_HOST_EXCHANGE) && d.batch != d.n_total, h->rounds_done);
}

int cmpc_di_rounds_log_range(cmpc_di_rounds* h, int* first_round, int* count) {
    return h ? log_range(h->ctx, h->log, first_round, count) : CMPC_ERR_ARG;
}

int cmpc_di_rounds_log_read(cmpc_di_rounds* h, int first_round, int count, const cmpc_rounds_log* o) {
    return h ? log_read(h->ctx, h->log, first_round, count, o) : CMPC_ERR_ARG;
}

}  // extern "C"
