// Consensus rounds behind a handle (include/cmpc.h, cmpc_lpv_rounds_* and cmpc_di_rounds_*): the device-resident
// loop of LPV_HP_N_main.py:96-117 for hosts that own no device memory (MATLAB through the MEX gateways, C).
// A handle owns this rank's agent state and the node-global exchange buffer in one device allocation; a round
// chains the C-ABI device entry points on the context's stream:
//   LPV: [cmpc_nbr_select_dev ->] cmpc_lpv_gather_dev -> cmpc_solve_lpv_batch_dev -> cmpc_lpv_advance_dev -> exchange
//   LPV, a consensus step (cmpc_lpv_rounds_step_consensus): [cmpc_nbr_select_dev ->] inner rounds of
//        cmpc_lpv_gather_dev -> cmpc_solve_lpv_batch_dev -> cmpc_lpv_publish_dev -> exchange -> 8-byte read-back at a
//        fixed state and linearisation, until the published positions agree -> cmpc_lpv_advance_dev
//   DI:  [cmpc_nbr_select_dev ->] cmpc_di_round_dev -> [cmpc_order_by_iters_dev ->] exchange
//   LIN: [cmpc_nbr_select_dev ->] cmpc_lin_round_dev -> [cmpc_order_by_iters_dev ->] exchange
//        (over a stage table: cmpc_lin_table_round_dev at the handle's time, which then moves on one stage)
//   LIN, a consensus step (cmpc_lin_rounds_step_consensus): [cmpc_nbr_select_dev ->] inner rounds of
//        cmpc_lin[_table]_build_dev -> cmpc_solve_mpc_batch_dev -> cmpc_lin_publish_dev -> exchange -> 4-byte
//        read-back, until the published positions agree -> cmpc_lin_advance_dev
//   LIN with 3-D positions (cmpc_lin_rounds_create3 / _create_table3): the same chains with cmpc_lin3_* for
//        cmpc_lin_* and cmpc_nbr_select3_dev for cmpc_nbr_select_dev, on exchange rows of 3 (N + 1) doubles
// where the exchange is a device copy (one rank), the RCCL all-gather of the context's communicator
// (cmpc_allgather_trajectories), or the host's (CMPC_ROUNDS_HOST_EXCHANGE).  With the log on
// (cmpc_*_rounds_log_enable) a round ends with cmpc_round_log_dev [-> cmpc_nbr_select_dev, nb = 1] into the
// handle's log ring, and an event pair brackets its solver call.
//
// What the families share lives once, in RoundsCore and the functions on it: the create checks, the device
// block, the re-selection, the exchange, get / set_traj, destroy and the log.  The DI and the linear-model (LIN)
// handles also share SolverRounds: the structured problem they hand cmpc_solve_mpc_batch_dev, the history ring,
// the step loop around the family's round entry, read and history.  The LPV step loop stays apart (its middle
// differs), and so does its error path: the LPV step returns at once, without a host synchronisation, and counts
// a round only after its exchange and log rows; the DI / LIN step counts a round as soon as its solver call and
// launch order are queued (its outputs exist whatever the exchange returns), leaves the loop at the first error
// and synchronises the host once before it returns the error.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "ctx.h"

namespace {

// One sub-array of a device block: where its address goes and its size.
struct Part {
    void** p;
    size_t bytes;
    template <class T>
    Part(T*& ptr, size_t count) : p(reinterpret_cast<void**>(&ptr)), bytes(sizeof(T) * count) {}
    size_t padded() const { return (bytes + 255) & ~size_t(255); }
};

// One hipMalloc for all `parts`, each 256-byte aligned, in list order (an empty part gets nullptr).  Sizes and
// addresses come from the same list.  Returns the block's bytes, 0 when the allocation failed (*mem = nullptr).
size_t device_block(char** mem, std::initializer_list<Part> parts) {
    size_t bytes = 0, off = 0;
    for (const Part& a : parts) bytes += a.padded();
    if (hipMalloc(mem, bytes) != hipSuccess) {
        *mem = nullptr;
        return 0;
    }
    for (const Part& a : parts) {
        *a.p = a.bytes ? *mem + off : nullptr;
        off += a.padded();
    }
    return bytes;
}

// The experiment log of a handle (cmpc_*_rounds_log_*): a device ring of `capacity` rounds, round r in row
// r % capacity, and an event pair per row around the round's solver call.  A block of its own, made by
// log_enable after create and freed by destroy.
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

}  // namespace

// What both handles are made of.
struct RoundsCore {
    cmpc_ctx* ctx = nullptr;
    cmpc_lpv_rounds_dims d{};  // n_total, batch, self_offset, N, nb, flags: what both families' dims begin with
    cmpc_opts opts{};
    int rounds_done = 0;       // since create (the log's round numbers)
    RoundLog* log = nullptr;   // cmpc_*_rounds_log_enable
    char* mem = nullptr;       // the device block of everything below and of the family's own arrays
    double *traj_all = nullptr, *traj_local = nullptr;
    int* nbr = nullptr;
    // the latest consensus step (cmpc_lin_rounds_step_consensus, cmpc_lpv_rounds_step_consensus): the last inner
    // round's verdicts and its two counts (not close; LPV: infeasible) on the device, the node-wide not-close count
    // of every inner round and the loop's outcome on the host
    int *close = nullptr, *counts = nullptr;
    double* delta = nullptr;
    std::vector<int> trace;
    bool agreed = false;

    bool sharded() const { return d.batch != d.n_total; }
    bool host_exchange() const { return d.flags & CMPC_ROUNDS_HOST_EXCHANGE; }
    int pos_dim = 2;  // coordinates of a position: 3 on a handle of cmpc_lin_rounds_create3 / _create_table3
    size_t traj_row() const { return (size_t)pos_dim * (d.N + 1); }  // doubles of one agent's predicted positions
    // cmpc_nbr_select_dev on the exchange buffer, by its width
    int select(const cmpc_nbr_dims* sd, int* nbr_out, double* dist2, hipStream_t s) const {
        return pos_dim == 3 ? cmpc_nbr_select3_dev(ctx, sd, traj_all, nbr_out, dist2, s)
                            : cmpc_nbr_select_dev(ctx, sd, traj_all, nbr_out, dist2, s);
    }
};

struct cmpc_lpv_rounds : RoundsCore {
    cmpc_lpv_params prm{};
    double seg[4][CMPC_MAX_SEG]{};  // copy of the track table: s0, len, curv, half_width
    cmpc_track track{};
    int last_rows = 0;              // N + 1 in the first round, N afterwards (LPV_HP_N_main.py:115)
    double *x0 = nullptr, *x_last = nullptr, *u_last = nullptr, *u_old = nullptr, *pose = nullptr,
           *x_agents = nullptr, *z = nullptr, *planes = nullptr, *kkt = nullptr, *x_dense = nullptr;
    int *iters = nullptr, *status = nullptr, *infeasible = nullptr;
};

// What the handles around cmpc_solve_mpc_batch_dev (DI, LIN) are made of.
struct SolverRounds : RoundsCore {
    int history = 1;  // round r writes row r % history of kkt / iters / status
    cmpc_mpc_dims md{};
    // copy of the batch-shared weights (cmpc_mpc_weights holds host pointers)
    double Q[CMPC_MAX_NX * CMPC_MAX_NX]{}, R[CMPC_MAX_NU * CMPC_MAX_NU]{}, dR[CMPC_MAX_NU * CMPC_MAX_NU]{},
        Qs[CMPC_MAX_NS]{}, u_ub[CMPC_MAX_NU]{}, u_lb[CMPC_MAX_NU]{};
    int row_slack[CMPC_MAX_MC]{}, row_sign[CMPC_MAX_MC]{};
    cmpc_mpc_weights w{};
    double *A = nullptr, *B = nullptr, *x0 = nullptr, *u_prev = nullptr, *qlin = nullptr, *C = nullptr, *h = nullptr,
           *z = nullptr, *kkt = nullptr;
    int *iters = nullptr, *status = nullptr, *order = nullptr;
};

struct cmpc_di_rounds : SolverRounds {
    cmpc_di_params prm{};
    double* lane = nullptr;
};

struct cmpc_lin_rounds : SolverRounds {
    cmpc_lin_params prm{};
    cmpc_lin3_params prm3{};  // pos_dim == 3: the rounds call the cmpc_lin3_* entries with it
    int mo = 0;
    // the own data, only read by the rounds: the fixed window (N + 1 / N / N stages, uploaded once), or the qlin /
    // C / h rows of a stage table (T stages each)
    double *qlin_own = nullptr, *C_own = nullptr, *h_own = nullptr;
    // the stage table of cmpc_lin_rounds_create_table (T == 0: a fixed-window handle) and the next round's time
    int T = 0, mode = CMPC_TABLE_HOLD, t = 0;
    double *A_tab = nullptr, *B_tab = nullptr;  // T stages; the round gathers their window into A, B
};

namespace {

size_t nz_lpv(int N) { return 12 * (size_t)(N + 1) + 4 * (size_t)N; }
size_t nz_mpc(const cmpc_mpc_dims& d) { return (size_t)(d.nx + d.ns) * (d.N + 1) + 2 * (size_t)d.nu * d.N; }

// ---- create ----

// The create checks the families share (`nbr`: init->nbr; `own_rows`: the stage rows before the nb planes);
// CMPC_OK, or CMPC_ERR_ARG with the message set.
int check_create(cmpc_ctx* ctx, const cmpc_lpv_rounds_dims& d, int known_flags, const int* nbr, const cmpc_opts* opts,
                 int own_rows = 4) {
    if (d.N < 1 || d.nb < 0 || own_rows + d.nb > CMPC_MAX_MC || d.batch < 1 || d.n_total < d.batch || d.self_offset < 0 ||
        d.self_offset + d.batch > d.n_total)
        return fail(ctx, CMPC_ERR_ARG, "bad rounds dimensions (1 <= batch, self_offset + batch <= n_total, nb <= 12)");
    if (d.flags & ~known_flags) return fail(ctx, CMPC_ERR_ARG, "unknown rounds flag");
    if ((d.flags & CMPC_ROUNDS_RESELECT) && d.nb >= d.n_total)
        return fail(ctx, CMPC_ERR_ARG, "CMPC_ROUNDS_RESELECT selects nb < n_total neighbours");
    if (d.nb > 0 && !nbr) return fail(ctx, CMPC_ERR_ARG, "null initial state");
    if (d.batch != d.n_total && !(d.flags & CMPC_ROUNDS_HOST_EXCHANGE) &&
        (!ctx->comm || (long)ctx->nranks * d.batch != d.n_total || ctx->rank * d.batch != d.self_offset))
        return fail(ctx, CMPC_ERR_ARG,
                    "a sharded population exchanges over the context's communicator (cmpc_comm_init: equal "
                    "contiguous shards in rank order) or the host's (CMPC_ROUNDS_HOST_EXCHANGE)");
    for (int i = 0; i < d.batch * d.nb; ++i)
        if (nbr[i] < 0 || nbr[i] >= d.n_total) return fail(ctx, CMPC_ERR_ARG, "neighbour index out of range");
    if (opts && (opts->flags & ~CMPC_FLAG_ALL)) return fail(ctx, CMPC_ERR_ARG, "unknown option flag");
    return CMPC_OK;
}

void core_init(RoundsCore* h, cmpc_ctx* ctx, const cmpc_lpv_rounds_dims& d, const cmpc_opts* opts) {
    h->ctx = ctx;
    h->d = d;
    if (opts) h->opts = *opts;
    h->opts.stamps = nullptr;
    h->opts.order = nullptr;
}

hipError_t upload(void* dst, const void* src, size_t bytes, hipStream_t s) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
}

// The end of both creates, after the family's uploads (`e`: their result): this rank's rows of the exchange
// buffer -> traj_local (an agent that is not advanced keeps its initial ones), and the host synchronisation.
hipError_t finish_uploads(RoundsCore* h, hipError_t e) {
    hipStream_t s = h->ctx->stream;
    const size_t own = 8 * h->traj_row() * h->d.batch;
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->traj_local, h->traj_all + h->traj_row() * h->d.self_offset, own, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

// CMPC_FLAG_LTI's condition on a host array of `batch` agents x `N` stages x `per` doubles: every stage of an
// agent bit-equal to its stage 0 (64-bit patterns: -0.0 is not +0.0), every entry finite
bool stages_lti(const double* a, size_t batch, size_t N, size_t per) {
    for (size_t b = 0; b < batch; ++b) {
        const double* a0 = a + b * N * per;
        for (size_t i = 0; i < N * per; ++i) {
            uint64_t u, v;
            std::memcpy(&u, a0 + i, 8);
            std::memcpy(&v, a0 + i % per, 8);
            if (u != v || !std::isfinite(a0[i])) return false;
        }
    }
    return true;
}

// ---- the parts of a round that both step loops call ----

// CMPC_ROUNDS_RESELECT: this round's neighbours are the nb nearest in the exchange buffer as it stands
int reselect(RoundsCore* h, hipStream_t s) {
    if (!(h->d.flags & CMPC_ROUNDS_RESELECT) || h->d.nb == 0) return CMPC_OK;
    const cmpc_nbr_dims sd{h->d.batch, h->d.N, h->d.nb, h->d.self_offset, h->d.n_total, 0, 0};
    return h->select(&sd, h->nbr, nullptr, s);
}

// traj_local -> every rank's traj_all; with the host's exchange (sharded) nothing: the host does it between steps
int exchange(RoundsCore* h, hipStream_t s) {
    const size_t count = h->traj_row() * h->d.batch;
    if (h->sharded())
        return h->host_exchange() ? CMPC_OK : cmpc_allgather_trajectories(h->ctx, h->traj_local, h->traj_all, count, s);
    const hipError_t e = hipMemcpyAsync(h->traj_all, h->traj_local, 8 * count, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? CMPC_OK : hip_fail(h->ctx, e, "rounds step: exchange");
}

// what both steps check before their loops
int check_step(const RoundsCore* h, int rounds) {
    if (rounds < 0) return fail(h->ctx, CMPC_ERR_ARG, "negative round count");
    if (h->host_exchange() && h->sharded() && rounds > 1)
        return fail(h->ctx, CMPC_ERR_ARG, "host exchange: one round per step (exchange between steps)");
    return CMPC_OK;
}

// ---- what the consensus steps of the families share (include/cmpc.h, cmpc_lin_rounds_step_consensus) ----

const cmpc_consensus_opts kConsensusDefaults{3, 2, 12, 0.01, 1e-5};  // NL_EU_N_main.py:102-104

// what both consensus steps check before their loops (`h` is not null)
int check_consensus(const RoundsCore* h, int steps, const cmpc_consensus_opts& o) {
    cmpc_ctx* ctx = h->ctx;
    if (steps < 0) return fail(ctx, CMPC_ERR_ARG, "negative step count");
    if (o.min_rounds < 1 || o.need < 1 || o.max_rounds < o.min_rounds)
        return fail(ctx, CMPC_ERR_ARG, "consensus: 1 <= min_rounds <= max_rounds, need >= 1");
    if (!(o.atol >= 0.0) || !(o.rtol >= 0.0)) return fail(ctx, CMPC_ERR_ARG, "atol and rtol: >= 0 (not NaN)");
    if (h->host_exchange() && h->sharded())
        return fail(ctx, CMPC_ERR_ARG, "host exchange: the exchange lies inside a consensus step");
    return CMPC_OK;
}

// The stopping rule (cmpc.scenarios.consensus_stop) over the inner rounds of one step: after(count) takes round
// j's node-wide not-close count and says whether the step stops there.
struct ConsensusLoop {
    const cmpc_consensus_opts& co;
    std::vector<int> trace;
    bool agreed = false;
    int streak = 0;
    bool after(int count) {
        trace.push_back(count);
        const int j = (int)trace.size();
        if (j >= 2) streak = count == 0 ? streak + 1 : 0;  // round 1 compares against the previous step's plan
        if (streak >= co.need) agreed = true;
        return j >= co.max_rounds || (agreed && j >= co.min_rounds);
    }
};

int consensus_read(RoundsCore* h, const cmpc_consensus_out* o) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!o) return fail(ctx, CMPC_ERR_ARG, "null output");
    if (o->cap < 0) return fail(ctx, CMPC_ERR_ARG, "negative cap");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = h->d.batch;
    if (o->close) HIP_TRY(hipMemcpyAsync(o->close, h->close, 4 * B, hipMemcpyDeviceToHost, s));
    if (o->delta) HIP_TRY(hipMemcpyAsync(o->delta, h->delta, 8 * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (o->inner_rounds) *o->inner_rounds = (int)h->trace.size();
    if (o->agreed) *o->agreed = h->agreed ? 1 : 0;
    if (o->not_close) std::copy_n(h->trace.begin(), std::min((size_t)o->cap, h->trace.size()), o->not_close);
    return CMPC_OK;
}

// ---- get_traj / set_traj / destroy ----

int copy_traj(RoundsCore* h, void* dst, const void* src, size_t agents, hipMemcpyKind kind) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!dst || !src) return fail(ctx, CMPC_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dst, src, 8 * h->traj_row() * agents, kind, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CMPC_OK;
}

int get_traj(RoundsCore* h, double* traj_local) {
    return h ? copy_traj(h, traj_local, h->traj_local, h->d.batch, hipMemcpyDeviceToHost) : CMPC_ERR_ARG;
}

int set_traj(RoundsCore* h, const double* traj_all) {
    return h ? copy_traj(h, h->traj_all, traj_all, h->d.n_total, hipMemcpyHostToDevice) : CMPC_ERR_ARG;
}

void log_free(RoundLog* lg) {
    if (!lg) return;
    for (hipEvent_t e : lg->ev) (void)hipEventDestroy(e);
    (void)hipFree(lg->mem);
    delete lg;
}

template <class Handle>
int destroy(Handle* h) {
    if (!h) return CMPC_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    log_free(h->log);
    (void)hipFree(h->mem);
    delete h;
    return CMPC_OK;
}

// ---- the log ----

// nx, nu, look_col, ns: the family's state and input widths, its look-ahead column and its slacks
int log_enable(RoundsCore* h, int capacity, int flags, int nx, int nu, int look_col, int ns = 3) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    const cmpc_lpv_rounds_dims& d = h->d;
    if (h->log) return fail(ctx, CMPC_ERR_ARG, "the log is already enabled");
    if (capacity < 1) return fail(ctx, CMPC_ERR_ARG, "log capacity < 1");
    if (flags & ~CMPC_LOG_SEPARATION) return fail(ctx, CMPC_ERR_ARG, "unknown log flag");
    const bool sep = flags & CMPC_LOG_SEPARATION;
    if (sep && d.n_total < 2) return fail(ctx, CMPC_ERR_ARG, "CMPC_LOG_SEPARATION needs n_total >= 2");
    if (sep && h->host_exchange() && h->sharded())
        return fail(ctx, CMPC_ERR_ARG,
                    "CMPC_LOG_SEPARATION on a sharded host-exchange handle: the other ranks' rows are stale when a "
                    "round ends");
    HIP_TRY(hipSetDevice(ctx->device));
    auto* lg = new RoundLog();
    lg->capacity = capacity;
    lg->flags = flags;
    lg->first = lg->end = h->rounds_done;
    lg->d = cmpc_log_dims{d.batch, nx, nu, ns, d.N, look_col};
    lg->sel = cmpc_nbr_dims{d.batch, d.N, 1, d.self_offset, d.n_total, 0, 0};
    const size_t rows = (size_t)capacity * d.batch, sep_rows = sep ? rows : 0;
    const size_t bytes = device_block(&lg->mem, {{lg->state, rows * nx}, {lg->u, rows * nu}, {lg->look, rows},
                                                 {lg->kkt, rows}, {lg->sep2, sep_rows}, {lg->iters, rows},
                                                 {lg->status, rows}, {lg->nearest, sep_rows}});
    if (!bytes) {
        log_free(lg);
        return fail(ctx, CMPC_ERR_NOMEM, "device allocation of the log ring failed");
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
    h->log = lg;
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

// round r's rows, stream-ordered after its exchange; nothing with the log off
int log_round(RoundsCore* h, int r, const double* z, const double* kkt, const int* iters, const int* status,
              hipStream_t s) {
    RoundLog* lg = h->log;
    if (!lg) return CMPC_OK;
    const size_t row = (size_t)(r % lg->capacity) * lg->d.batch;
    const cmpc_log_row dst{lg->state + row * lg->d.nx, lg->u + row * lg->d.nu, lg->look + row,
                           lg->kkt + row, lg->iters + row, lg->status + row};
    int rc = cmpc_round_log_dev(h->ctx, &lg->d, z, kkt, iters, status, &dst, s);
    if (rc == CMPC_OK && (lg->flags & CMPC_LOG_SEPARATION))
        rc = h->select(&lg->sel, lg->nearest + row, lg->sep2 + row, s);
    if (rc != CMPC_OK) return rc;
    if (r != lg->end) lg->first = r;  // a round in between went unlogged (its exchange failed): the log restarts here
    lg->end = r + 1;
    return CMPC_OK;
}

int log_range(RoundsCore* h, int* first_round, int* count) {
    if (!h) return CMPC_ERR_ARG;
    const RoundLog* lg = h->log;
    if (!lg) return fail(h->ctx, CMPC_ERR_ARG, "the log is not enabled (log_enable)");
    const int lo = std::max(lg->first, lg->end - lg->capacity);
    if (first_round) *first_round = lo;
    if (count) *count = lg->end - lo;
    return CMPC_OK;
}

int log_read(RoundsCore* h, int first_round, int count, const cmpc_rounds_log* o) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    const RoundLog* lg = h->log;
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

// ---- the handles around cmpc_solve_mpc_batch_dev (DI, LIN) ----

// the batch-shared weights of `w` (md is set), copied into the handle
void copy_weights(SolverRounds* h, const cmpc_mpc_weights* w) {
    const int nx = h->md.nx, nu = h->md.nu, ns = h->md.ns, mc = h->md.mc;
    std::memcpy(h->Q, w->Q, sizeof(double) * nx * nx);
    std::memcpy(h->R, w->R, sizeof(double) * nu * nu);
    std::memcpy(h->dR, w->dR, sizeof(double) * nu * nu);
    std::memcpy(h->Qs, w->Qs, sizeof(double) * ns);
    std::memcpy(h->u_ub, w->u_ub, sizeof(double) * nu);
    std::memcpy(h->u_lb, w->u_lb, sizeof(double) * nu);
    std::memcpy(h->row_slack, w->row_slack, sizeof(int) * mc);
    std::memcpy(h->row_sign, w->row_sign, sizeof(int) * mc);
    h->w = cmpc_mpc_weights{h->Q, h->R, h->dR, h->Qs, h->u_ub, h->u_lb, h->row_slack, h->row_sign};
}

// The step loop: `round_call(data, out, stream)` is the family's round entry (build, solve, advance) on the
// handle's buffers, `out` this round's row of the history ring; `where`: the entry's name for a device error.
template <class Round>
int step_rounds(SolverRounds* h, int rounds, int* rounds_done, const char* where, Round round_call) {
    cmpc_ctx* ctx = h->ctx;
    if (rounds_done) *rounds_done = 0;
    int done = 0, rc;
    if ((rc = check_step(h, rounds)) != CMPC_OK) return rc;
    const bool lpt = h->d.flags & CMPC_ROUNDS_LPT;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const cmpc_mpc_data din{h->A, h->B, h->x0, h->u_prev, h->qlin, h->C, h->h};
    for (int r = 0; r < rounds && rc == CMPC_OK; ++r) {
        const int round = h->rounds_done;
        const size_t slot = (size_t)(round % h->history) * h->d.batch;  // this round's row of the history ring
        const cmpc_mpc_out dout{h->z, h->kkt + slot, h->iters + slot, h->status + slot};
        if ((rc = reselect(h, s)) != CMPC_OK) break;
        h->opts.order = (lpt && round > 0) ? h->order : nullptr;
        hipError_t ev = log_mark(h->log, round, 0, s);
        if (ev == hipSuccess) {
            if ((rc = round_call(&din, &dout, s)) != CMPC_OK) {
                log_abandon(h->log, round);
                break;
            }
            ev = log_mark(h->log, round, 1, s);
        }
        if (ev != hipSuccess) {
            rc = hip_fail(ctx, ev, where);
            break;
        }
        // the next round's launch order, stream-ordered after this solve
        if (lpt && (rc = cmpc_order_by_iters_dev(ctx, h->d.batch, h->iters + slot, h->order, s)) != CMPC_OK) break;
        ++h->rounds_done;  // the round's outputs exist from here on, whatever the exchange returns
        ++done;
        // the log's rows of this round, from the history-ring row the solver wrote
        if ((rc = exchange(h, s)) == CMPC_OK)
            rc = log_round(h, round, h->z, h->kkt + slot, h->iters + slot, h->status + slot, s);
    }
    // one host synchronisation, also after an error: the rounds already queued have then finished
    const hipError_t e = hipStreamSynchronize(s);
    if (rounds_done) *rounds_done = done;
    if (rc != CMPC_OK) return rc;
    HIP_TRY(e);
    return CMPC_OK;
}

// Out: cmpc_di_rounds_out / cmpc_lin_rounds_out (the same members)
template <class Out>
int read_rounds(SolverRounds* h, const Out* o) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!o) return fail(ctx, CMPC_ERR_ARG, "null output");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = h->d.batch;
    const size_t slot = (size_t)((h->rounds_done > 0 ? h->rounds_done - 1 : 0) % h->history) * B;
    auto dn = [&](void* dst, const void* src, size_t b) { return hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, s); };
    if (o->z) HIP_TRY(dn(o->z, h->z, 8 * B * nz_mpc(h->md)));
    if (o->kkt) HIP_TRY(dn(o->kkt, h->kkt + slot, 8 * B));
    if (o->iters) HIP_TRY(dn(o->iters, h->iters + slot, 4 * B));
    if (o->status) HIP_TRY(dn(o->status, h->status + slot, 4 * B));
    if (o->x0) HIP_TRY(dn(o->x0, h->x0, 8 * B * h->md.nx));
    if (o->u_prev) HIP_TRY(dn(o->u_prev, h->u_prev, 8 * B * h->md.nu));
    if (o->nbr && h->d.nb) HIP_TRY(dn(o->nbr, h->nbr, 4 * B * h->d.nb));
    HIP_TRY(hipStreamSynchronize(s));
    return CMPC_OK;
}

int history_rounds(SolverRounds* h, int first_round, int count, double* kkt, int* iters, int* status) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (first_round < 0 || count < 0 || (long long)first_round + count > h->rounds_done)
        return fail(ctx, CMPC_ERR_ARG, "history: a round that has not run yet");
    if (count > 0 && first_round < h->rounds_done - h->history)
        return fail(ctx, CMPC_ERR_ARG, "history: a round the ring has already overwritten (dims.history rounds are kept)");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = h->d.batch;
    for (int i = 0; i < count; ++i) {
        const size_t slot = (size_t)((first_round + i) % h->history) * B;
        if (kkt) HIP_TRY(hipMemcpyAsync(kkt + i * B, h->kkt + slot, 8 * B, hipMemcpyDeviceToHost, s));
        if (iters) HIP_TRY(hipMemcpyAsync(iters + i * B, h->iters + slot, 4 * B, hipMemcpyDeviceToHost, s));
        if (status) HIP_TRY(hipMemcpyAsync(status + i * B, h->status + slot, 4 * B, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return CMPC_OK;
}

// ---- the linear-model handle's two creates ----

// What cmpc_lin_rounds_create and cmpc_lin_rounds_create_table hand lin_create: HOST pointers.  T == 0: A, B,
// qlin, C, h are the fixed window (N, N, N + 1, N, N stages); T >= 1: the stage table (T stages each).
struct LinInit {
    int T, mode, t0;
    const double *A, *B, *qlin, *C, *h, *x0, *u_prev;
    const int* nbr;
    const double* traj;
};

void set_position(cmpc_lin_rounds* h, const cmpc_lin_params& prm) { h->prm = prm; }
void set_position(cmpc_lin_rounds* h, const cmpc_lin3_params& prm) {
    h->prm = cmpc_lin_params{prm.ix, prm.iy, prm.min_dist, prm.wq};
    h->prm3 = prm;
    h->pos_dim = 3;
}

// Prm: cmpc_lin_params, or cmpc_lin3_params (in.traj is then n_total x (N+1) x 3)
template <class Prm>
int lin_create(cmpc_ctx* ctx, const Prm* prm, const cmpc_mpc_weights* w, const cmpc_lin_rounds_dims* dims,
               const LinInit& in, bool table, const cmpc_opts* opts, cmpc_lin_rounds** out) {
    const cmpc_lpv_rounds_dims d{dims->n_total, dims->batch, dims->self_offset, dims->N, dims->nb, dims->flags};
    const cmpc_lin_dims ld{d.batch, d.N, d.nb, d.self_offset, dims->nx, dims->mo};
    cmpc::LinConst lc;
    int rc = lin_const(ctx, prm, &ld, &lc);  // the family's own dimension rules first: mo is checked before it is used
    if (rc != CMPC_OK) return rc;
    if (dims->nu < 1 || dims->nu > CMPC_MAX_NU || dims->ns < 0 || dims->ns > CMPC_MAX_NS)
        return fail(ctx, CMPC_ERR_ARG, "bad linear-model dimensions (0 <= ns <= 4, 1 <= nu <= 4)");
    if (table && (in.T < 1 || (in.mode != CMPC_TABLE_HOLD && in.mode != CMPC_TABLE_PERIODIC) || in.t0 < 0 || in.t0 >= in.T))
        return fail(ctx, CMPC_ERR_ARG, "bad stage table (T >= 1, mode CMPC_TABLE_HOLD or CMPC_TABLE_PERIODIC, 0 <= t0 < T)");
    rc = check_create(ctx, d, CMPC_ROUNDS_HOST_EXCHANGE | CMPC_ROUNDS_NO_HALT | CMPC_ROUNDS_RESELECT | CMPC_ROUNDS_LPT,
                      in.nbr, opts, dims->mo);
    if (rc != CMPC_OK) return rc;
    if (dims->history < 0) return fail(ctx, CMPC_ERR_ARG, "negative history");
    if (!w->Q || !w->R || !w->dR || (dims->ns && !w->Qs) || !w->u_ub || !w->u_lb ||
        (dims->mo + d.nb && (!w->row_slack || !w->row_sign)))
        return fail(ctx, CMPC_ERR_ARG, "null weights");
    if (!in.A || !in.B || !in.x0 || !in.u_prev || !in.qlin || !in.traj || (dims->mo && (!in.C || !in.h)))
        return fail(ctx, CMPC_ERR_ARG, "null initial state");
    HIP_TRY(hipSetDevice(ctx->device));

    auto* h = new cmpc_lin_rounds();
    core_init(h, ctx, d, opts);
    set_position(h, *prm);
    h->mo = dims->mo;
    h->history = std::max(dims->history, 1);
    if (table) {
        h->T = in.T;
        h->mode = in.mode;
        h->t = in.t0;
    }
    const int nx = dims->nx, nu = dims->nu, mo = dims->mo, mc = mo + d.nb;
    h->md = cmpc_mpc_dims{nx, nu, d.N, dims->ns, mc, d.batch};
    // the stages of the caller's model, cost and row arrays
    const size_t B = d.batch, N = d.N, SA = table ? in.T : N, Sq = table ? in.T : N + 1, SC = table ? in.T : N;
    // time-invariant agents: the promise the solver may use.  The fixed window never changes after this; of a
    // table every row has to agree, since any of them may enter a window (cmpc_lin_rounds_table_write withdraws it)
    if (stages_lti(in.A, B, SA, (size_t)nx * nx) && stages_lti(in.B, B, SA, (size_t)nx * nu))
        h->opts.flags |= CMPC_FLAG_LTI;
    copy_weights(h, w);

    const size_t nb1 = d.nb ? d.nb : 1, T = d.n_total, row = h->traj_row(), H = h->history;
    const size_t nA = B * N * nx * nx, nB = B * N * nx * nu, nq = B * (N + 1) * nx;
    const size_t uA = B * SA * nx * nx, uB = B * SA * nx * nu, uq = B * Sq * nx, uC = B * SC * mo * nx, uh = B * SC * mo;
    const size_t bytes = device_block(
        &h->mem, {{h->A, nA}, {h->B, nB}, {h->x0, B * nx}, {h->u_prev, B * nu}, {h->qlin_own, uq}, {h->C_own, uC},
                  {h->h_own, uh}, {h->traj_all, T * row}, {h->traj_local, B * row}, {h->qlin, nq},
                  {h->C, B * N * mc * nx}, {h->h, B * N * mc}, {h->z, B * nz_mpc(h->md)}, {h->kkt, H * B},
                  {h->nbr, B * nb1}, {h->iters, H * B}, {h->status, H * B}, {h->order, B},
                  {h->A_tab, table ? uA : 0}, {h->B_tab, table ? uB : 0}, {h->close, B}, {h->delta, B},
                  {h->counts, 2}});
    if (!bytes) {
        delete h;
        return fail(ctx, CMPC_ERR_NOMEM, "device allocation of the rounds state failed");
    }
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemsetAsync(h->mem, 0, bytes, s);  // a read before the first round returns zeros
    if (e == hipSuccess) e = upload(table ? h->A_tab : h->A, in.A, 8 * uA, s);
    if (e == hipSuccess) e = upload(table ? h->B_tab : h->B, in.B, 8 * uB, s);
    if (e == hipSuccess) e = upload(h->x0, in.x0, 8 * B * nx, s);
    if (e == hipSuccess) e = upload(h->u_prev, in.u_prev, 8 * B * nu, s);
    if (e == hipSuccess) e = upload(h->qlin_own, in.qlin, 8 * uq, s);
    if (e == hipSuccess && mo) e = upload(h->C_own, in.C, 8 * uC, s);
    if (e == hipSuccess && mo) e = upload(h->h_own, in.h, 8 * uh, s);
    if (e == hipSuccess) e = upload(h->traj_all, in.traj, 8 * T * row, s);
    if (e == hipSuccess && d.nb) e = upload(h->nbr, in.nbr, 4 * B * d.nb, s);
    if ((e = finish_uploads(h, e)) != hipSuccess) {
        (void)hipFree(h->mem);
        delete h;
        return hip_fail(ctx, e, "cmpc_lin_rounds_create: upload");
    }
    *out = h;
    return CMPC_OK;
}

}  // namespace

extern "C" {

// ---- the reference's LPV agents (cmpc_lpv_rounds_*) ----

int cmpc_lpv_rounds_create(cmpc_ctx* ctx, const cmpc_lpv_params* prm, const cmpc_track* track,
                           const cmpc_lpv_rounds_dims* dims, const cmpc_lpv_rounds_init* in, const cmpc_opts* opts,
                           cmpc_lpv_rounds** out) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!out || !prm || !track || !dims || !in) return fail(ctx, CMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const cmpc_lpv_rounds_dims& d = *dims;
    const int rc = check_create(ctx, d, CMPC_ROUNDS_HOST_EXCHANGE | CMPC_ROUNDS_NO_HALT | CMPC_ROUNDS_RESELECT, in->nbr,
                                opts);
    if (rc != CMPC_OK) return rc;
    if (track->nseg < 1 || track->nseg > CMPC_MAX_SEG) return fail(ctx, CMPC_ERR_UNSUPPORTED, "track has 1..32 segments");
    if (!in->x0 || !in->x_last || !in->u_last) return fail(ctx, CMPC_ERR_ARG, "null initial state");
    if (!in->traj && d.batch != d.n_total)
        return fail(ctx, CMPC_ERR_ARG, "a sharded population needs the initial exchange buffer (init->traj)");
    HIP_TRY(hipSetDevice(ctx->device));

    auto* h = new cmpc_lpv_rounds();
    core_init(h, ctx, d, opts);
    h->prm = *prm;
    h->last_rows = d.N + 1;
    const int ns = track->nseg;
    std::memcpy(h->seg[0], track->s0, sizeof(double) * ns);
    std::memcpy(h->seg[1], track->len, sizeof(double) * ns);
    std::memcpy(h->seg[2], track->curv, sizeof(double) * ns);
    std::memcpy(h->seg[3], track->half_width, sizeof(double) * ns);
    h->track = cmpc_track{ns, h->seg[0], h->seg[1], h->seg[2], h->seg[3]};

    const size_t B = d.batch, N = d.N, nb1 = d.nb ? d.nb : 1, T = d.n_total, row = h->traj_row();
    if (!device_block(&h->mem, {{h->x0, B * 9}, {h->x_last, B * (N + 1) * 9}, {h->u_last, B * N * 2}, {h->u_old, B * 2},
                                {h->traj_all, T * row}, {h->traj_local, B * row}, {h->pose, B * row},
                                {h->x_agents, B * row * nb1}, {h->z, B * nz_lpv(d.N)}, {h->planes, B * N * 3 * nb1},
                                {h->kkt, B}, {h->x_dense, B * N * 9}, {h->nbr, B * nb1}, {h->iters, B}, {h->status, B},
                                {h->infeasible, B}, {h->close, B}, {h->delta, B}, {h->counts, 2}})) {
        delete h;
        return fail(ctx, CMPC_ERR_NOMEM, "device allocation of the rounds state failed");
    }
    hipStream_t s = ctx->stream;
    hipError_t e = upload(h->x0, in->x0, 8 * B * 9, s);
    if (e == hipSuccess) e = upload(h->x_last, in->x_last, 8 * B * (N + 1) * 9, s);
    if (e == hipSuccess) e = upload(h->u_last, in->u_last, 8 * B * N * 2, s);
    if (e == hipSuccess) e = in->u_old ? upload(h->u_old, in->u_old, 8 * B * 2, s) : hipMemsetAsync(h->u_old, 0, 8 * B * 2, s);
    if (e == hipSuccess && d.nb) e = upload(h->nbr, in->nbr, 4 * B * d.nb, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->planes, 0, 8 * B * N * 3 * nb1, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->close, 0, 4 * B, s);  // a read before the first consensus step: zeros
    if (e == hipSuccess) e = hipMemsetAsync(h->delta, 0, 8 * B, s);
    if (e == hipSuccess && in->traj) e = upload(h->traj_all, in->traj, 8 * T * row, s);
    if (e == hipSuccess && !in->traj)  // the reference's initial `agents` = the predictions' X, Y (misc.py:155-165)
        e = hipMemcpy2DAsync(h->traj_all, 16, h->x_last + 7, 72, 16, B * (N + 1), hipMemcpyDeviceToDevice, s);
    if ((e = finish_uploads(h, e)) != hipSuccess) {
        (void)hipFree(h->mem);
        delete h;
        return hip_fail(ctx, e, "cmpc_lpv_rounds_create: upload");
    }
    *out = h;
    return CMPC_OK;
}

// Before the first advance of a handle: Last_xPredicted goes from N + 1 rows per agent to N dense ones.  The
// advance rewrites each agent's dense slot from its solution, but an agent it does not advance (no finite
// solution) must find its own previous rows there, not bytes of the (N + 1)-row layout: compact the layout first
// (rows 0..N-1 of each agent).  Nothing once last_rows is N.
static int compact_x_last(cmpc_lpv_rounds* h, hipStream_t s) {
    cmpc_ctx* ctx = h->ctx;
    if (h->last_rows != h->d.N + 1) return CMPC_OK;
    const size_t w = 8 * (size_t)h->d.N * 9;
    HIP_TRY(hipMemcpy2DAsync(h->x_dense, w, h->x_last, w + 72, w, h->d.batch, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->x_last, h->x_dense, w * h->d.batch, hipMemcpyDeviceToDevice, s));
    return CMPC_OK;
}

int cmpc_lpv_rounds_step(cmpc_lpv_rounds* h, int rounds, int* rounds_done, int* infeasible) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    int done = 0, bad = 0, rc;
    if ((rc = check_step(h, rounds)) != CMPC_OK) return rc;
    const bool halt = !(h->d.flags & CMPC_ROUNDS_NO_HALT);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int nb = h->d.nb;
    const cmpc_di_dims rd{h->d.batch, h->d.N, nb, h->d.self_offset};
    for (int r = 0; r < rounds; ++r) {
        if ((rc = reselect(h, s)) != CMPC_OK) return rc;
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
        if ((rc = compact_x_last(h, s)) != CMPC_OK) return rc;
        if ((rc = cmpc_lpv_advance_dev(ctx, &rd, h->z, h->x0, h->x_last, h->u_last, h->u_old, h->traj_local, h->status,
                                       h->infeasible, s)) != CMPC_OK)
            return rc;
        h->last_rows = h->d.N;  // x_old = xPred[1:] from now on (LPV_HP_N_main.py:115)
        if ((rc = exchange(h, s)) != CMPC_OK) return rc;
        // the node's infeasible count, not this rank's: the reference's loop quits for every agent
        // at once (LPV_HP_N_main.py:102-111), so every rank must take the same halt decision (a
        // rank that broke alone would leave the others waiting in the next round's all-gather).
        // The host exchange runs one round per step: its caller combines the counts it returns.
        if (h->sharded() && !h->host_exchange() && (rc = cmpc_comm_sum_i32(ctx, h->infeasible, 1, s)) != CMPC_OK)
            return rc;
        // the log's rows of this round (a round that halts the loop below has run, and is logged)
        if ((rc = log_round(h, h->rounds_done, h->z, h->kkt, h->iters, h->status, s)) != CMPC_OK) return rc;
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

// ---- consensus steps (include/cmpc.h, cmpc_lpv_rounds_step_consensus) ----

// One consensus step: inner rounds of gather, solve, publish and exchange at the handle's state and linearisation
// (x0, x_last, u_last, u_old, last_rows: untouched by inner rounds) until the stopping rule or the halt rule ends
// them, then the advance.  *inner: the inner rounds of a step that was counted (0: it was not); *bad: the node-wide
// infeasible count of the last inner round run.  Returns at the first error; the caller synchronises.
static int lpv_consensus_step(cmpc_lpv_rounds* h, const cmpc_consensus_opts& co, hipStream_t s, int* inner, int* bad) {
    cmpc_ctx* ctx = h->ctx;
    *inner = 0;
    const bool halt = !(h->d.flags & CMPC_ROUNDS_NO_HALT);
    const int round = h->rounds_done, nb = h->d.nb;
    const cmpc_di_dims rd{h->d.batch, h->d.N, nb, h->d.self_offset};
    const cmpc_lpv_dims ld{h->d.batch, h->d.N, nb, h->last_rows};
    const cmpc_lpv_data din{h->x0, h->x_last, h->u_last, h->u_old, nb ? h->x_agents : nullptr, h->pose};
    const cmpc_lpv_out dout{h->z, nb ? h->planes : nullptr, h->kkt, h->iters, h->status};
    int rc;
    if ((rc = reselect(h, s)) != CMPC_OK) return rc;
    HIP_TRY(log_mark(h->log, round, 0, s));
    ConsensusLoop loop{co};
    int j = 0;
    for (;;) {
        ++j;
        rc = cmpc_lpv_gather_dev(ctx, &rd, h->nbr, h->traj_all, nb ? h->x_agents : nullptr, h->pose, s);
        if (rc == CMPC_OK) rc = cmpc_solve_lpv_batch_dev(ctx, &h->prm, &h->track, &ld, &din, &dout, &h->opts, s);
        if (rc != CMPC_OK) {
            log_abandon(h->log, round);
            return rc;
        }
        HIP_TRY(hipMemsetAsync(h->counts, 0, 2 * sizeof(int), s));
        if ((rc = cmpc_lpv_publish_dev(ctx, &rd, h->z, h->traj_all, h->status, co.atol, co.rtol, h->traj_local, h->close,
                                       h->delta, h->counts, s)) != CMPC_OK)
            return rc;
        if ((rc = exchange(h, s)) != CMPC_OK) return rc;
        // the node's counts, not this rank's: every rank must leave the loop after the same inner round (a rank
        // that left alone would keep the others waiting in the next all-gather)
        if (h->sharded() && (rc = cmpc_comm_sum_i32(ctx, h->counts, 2, s)) != CMPC_OK) return rc;
        int counts[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(counts, h->counts, sizeof counts, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        *bad = counts[1];
        const bool stop = loop.after(counts[0]);
        if (stop || (halt && counts[1] > 0)) break;  // the reference stops the experiment at an infeasible agent
    }
    HIP_TRY(log_mark(h->log, round, 1, s));
    if ((rc = compact_x_last(h, s)) != CMPC_OK) return rc;
    // the state and the linearisation point from the final z; traj_local again, with the values the last inner
    // round exchanged (the publish has counted: no status here)
    if ((rc = cmpc_lpv_advance_dev(ctx, &rd, h->z, h->x0, h->x_last, h->u_last, h->u_old, h->traj_local, nullptr,
                                   nullptr, s)) != CMPC_OK)
        return rc;
    h->last_rows = h->d.N;
    if ((rc = log_round(h, round, h->z, h->kkt, h->iters, h->status, s)) != CMPC_OK) return rc;
    ++h->rounds_done;
    h->trace = std::move(loop.trace);
    h->agreed = loop.agreed;
    *inner = j;
    return CMPC_OK;
}

int cmpc_lpv_rounds_step_consensus(cmpc_lpv_rounds* h, int steps, const cmpc_consensus_opts* co, int* steps_done,
                                   int* inner_total, int* infeasible) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    const cmpc_consensus_opts o = co ? *co : kConsensusDefaults;
    int done = 0, total = 0, bad = 0, rc;
    if ((rc = check_consensus(h, steps, o)) != CMPC_OK) return rc;
    const bool halt = !(h->d.flags & CMPC_ROUNDS_NO_HALT);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (int i = 0; i < steps && rc == CMPC_OK; ++i) {
        int inner = 0;
        rc = lpv_consensus_step(h, o, s, &inner, &bad);
        if (inner) ++done;
        total += inner;
        if (halt && bad) break;  // as cmpc_lpv_rounds_step after a round with an infeasible agent
    }
    // one more host synchronisation, also after an error: what was queued has then finished
    const hipError_t e = hipStreamSynchronize(s);
    if (steps_done) *steps_done = done;
    if (inner_total) *inner_total = total;
    if (infeasible) *infeasible = bad;
    if (rc != CMPC_OK) return rc;
    HIP_TRY(e);
    return CMPC_OK;
}

int cmpc_lpv_rounds_consensus_read(cmpc_lpv_rounds* h, const cmpc_consensus_out* o) { return consensus_read(h, o); }

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

int cmpc_lpv_rounds_get_traj(cmpc_lpv_rounds* h, double* traj_local) { return get_traj(h, traj_local); }
int cmpc_lpv_rounds_set_traj(cmpc_lpv_rounds* h, const double* traj_all) { return set_traj(h, traj_all); }
int cmpc_lpv_rounds_destroy(cmpc_lpv_rounds* h) { return destroy(h); }
int cmpc_lpv_rounds_log_enable(cmpc_lpv_rounds* h, int capacity, int flags) {
    return log_enable(h, capacity, flags, 9, 2, 6);
}
int cmpc_lpv_rounds_log_range(cmpc_lpv_rounds* h, int* first_round, int* count) {
    return log_range(h, first_round, count);
}
int cmpc_lpv_rounds_log_read(cmpc_lpv_rounds* h, int first_round, int count, const cmpc_rounds_log* o) {
    return log_read(h, first_round, count, o);
}

// ---- the synthetic double-integrator family (cmpc_di_rounds_*): what cmpc.rounds.DIRounds.step() chains ----

int cmpc_di_rounds_create(cmpc_ctx* ctx, const cmpc_di_params* prm, const cmpc_mpc_weights* w,
                          const cmpc_di_rounds_dims* dims, const cmpc_di_rounds_init* in, const cmpc_opts* opts,
                          cmpc_di_rounds** out) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!out || !prm || !w || !dims || !in) return fail(ctx, CMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const cmpc_lpv_rounds_dims d{dims->n_total, dims->batch, dims->self_offset, dims->N, dims->nb, dims->flags};
    const int rc = check_create(
        ctx, d, CMPC_ROUNDS_HOST_EXCHANGE | CMPC_ROUNDS_NO_HALT | CMPC_ROUNDS_RESELECT | CMPC_ROUNDS_LPT, in->nbr, opts);
    if (rc != CMPC_OK) return rc;
    if (prm->dim != 2 && prm->dim != 3) return fail(ctx, CMPC_ERR_ARG, "double-integrator agents have dim 2 or 3");
    if (dims->history < 0) return fail(ctx, CMPC_ERR_ARG, "negative history");
    if (!w->Q || !w->R || !w->dR || !w->Qs || !w->u_ub || !w->u_lb || !w->row_slack || !w->row_sign)
        return fail(ctx, CMPC_ERR_ARG, "null weights");
    if (!in->A || !in->B || !in->x0 || !in->u_prev || !in->lane || !in->traj)
        return fail(ctx, CMPC_ERR_ARG, "null initial state");
    HIP_TRY(hipSetDevice(ctx->device));

    auto* h = new cmpc_di_rounds();
    core_init(h, ctx, d, opts);
    h->prm = *prm;
    h->history = std::max(dims->history, 1);
    const int nx = 2 * prm->dim, nu = prm->dim, mc = 4 + d.nb;
    h->md = cmpc_mpc_dims{nx, nu, d.N, 3, mc, d.batch};
    // time-invariant agents (the handle never changes A or B after this): the promise the solver may use
    if (stages_lti(in->A, d.batch, d.N, (size_t)nx * nx) && stages_lti(in->B, d.batch, d.N, (size_t)nx * nu))
        h->opts.flags |= CMPC_FLAG_LTI;
    copy_weights(h, w);

    const size_t B = d.batch, N = d.N, nb1 = d.nb ? d.nb : 1, T = d.n_total, row = h->traj_row(), H = h->history;
    const size_t nA = B * N * nx * nx, nB = B * N * nx * nu;
    const size_t bytes = device_block(
        &h->mem, {{h->A, nA}, {h->B, nB}, {h->x0, B * nx}, {h->u_prev, B * nu}, {h->lane, B}, {h->traj_all, T * row},
                  {h->traj_local, B * row}, {h->qlin, B * (N + 1) * nx}, {h->C, B * N * mc * nx}, {h->h, B * N * mc},
                  {h->z, B * nz_mpc(h->md)}, {h->kkt, H * B}, {h->nbr, B * nb1}, {h->iters, H * B},
                  {h->status, H * B}, {h->order, B}});
    if (!bytes) {
        delete h;
        return fail(ctx, CMPC_ERR_NOMEM, "device allocation of the rounds state failed");
    }
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemsetAsync(h->mem, 0, bytes, s);  // a read before the first round returns zeros
    if (e == hipSuccess) e = upload(h->A, in->A, 8 * nA, s);
    if (e == hipSuccess) e = upload(h->B, in->B, 8 * nB, s);
    if (e == hipSuccess) e = upload(h->x0, in->x0, 8 * B * nx, s);
    if (e == hipSuccess) e = upload(h->u_prev, in->u_prev, 8 * B * nu, s);
    if (e == hipSuccess) e = upload(h->lane, in->lane, 8 * B, s);
    if (e == hipSuccess) e = upload(h->traj_all, in->traj, 8 * T * row, s);
    if (e == hipSuccess && d.nb) e = upload(h->nbr, in->nbr, 4 * B * d.nb, s);
    if ((e = finish_uploads(h, e)) != hipSuccess) {
        (void)hipFree(h->mem);
        delete h;
        return hip_fail(ctx, e, "cmpc_di_rounds_create: upload");
    }
    *out = h;
    return CMPC_OK;
}

int cmpc_di_rounds_step(cmpc_di_rounds* h, int rounds, int* rounds_done) {
    if (!h) return CMPC_ERR_ARG;
    const cmpc_di_dims rd{h->d.batch, h->d.N, h->d.nb, h->d.self_offset};
    return step_rounds(h, rounds, rounds_done, "cmpc_di_rounds_step: log event",
                       [&](const cmpc_mpc_data* din, const cmpc_mpc_out* dout, hipStream_t s) {
                           return cmpc_di_round_dev(h->ctx, &h->prm, &rd, h->nbr, h->lane, h->traj_all, &h->md, &h->w,
                                                    din, dout, &h->opts, h->traj_local, s);
                       });
}

int cmpc_di_rounds_read(cmpc_di_rounds* h, const cmpc_di_rounds_out* o) { return read_rounds(h, o); }

int cmpc_di_rounds_history(cmpc_di_rounds* h, int first_round, int count, double* kkt, int* iters, int* status) {
    return history_rounds(h, first_round, count, kkt, iters, status);
}

int cmpc_di_rounds_get_traj(cmpc_di_rounds* h, double* traj_local) { return get_traj(h, traj_local); }
int cmpc_di_rounds_set_traj(cmpc_di_rounds* h, const double* traj_all) { return set_traj(h, traj_all); }
int cmpc_di_rounds_destroy(cmpc_di_rounds* h) { return destroy(h); }
int cmpc_di_rounds_log_enable(cmpc_di_rounds* h, int capacity, int flags) {
    return h ? log_enable(h, capacity, flags, h->md.nx, h->md.nu, 0) : CMPC_ERR_ARG;
}
int cmpc_di_rounds_log_range(cmpc_di_rounds* h, int* first_round, int* count) { return log_range(h, first_round, count); }
int cmpc_di_rounds_log_read(cmpc_di_rounds* h, int first_round, int count, const cmpc_rounds_log* o) {
    return log_read(h, first_round, count, o);
}

// ---- agents of any linear model (cmpc_lin_rounds_*): the DI handle with the caller's own rows and cost ----

int cmpc_lin_rounds_create(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_mpc_weights* w,
                           const cmpc_lin_rounds_dims* dims, const cmpc_lin_rounds_init* in, const cmpc_opts* opts,
                           cmpc_lin_rounds** out) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!out || !prm || !w || !dims || !in) return fail(ctx, CMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const LinInit li{0, 0, 0, in->A, in->B, in->qlin_own, in->C_own, in->h_own, in->x0, in->u_prev, in->nbr, in->traj};
    return lin_create(ctx, prm, w, dims, li, false, opts, out);
}

// the same handle over a stage table: the round's window slides one stage per round
int cmpc_lin_rounds_create_table(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_mpc_weights* w,
                                 const cmpc_lin_rounds_dims* dims, const cmpc_lin_rounds_table_init* in,
                                 const cmpc_opts* opts, cmpc_lin_rounds** out) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!out || !prm || !w || !dims || !in) return fail(ctx, CMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const LinInit li{in->T, in->mode, in->t0, in->A, in->B, in->qlin, in->C, in->h, in->x0, in->u_prev, in->nbr, in->traj};
    return lin_create(ctx, prm, w, dims, li, true, opts, out);
}

// ... and both with 3-D positions (include/cmpc.h, cmpc_lin3_*): the same handle, its exchange rows x 3
int cmpc_lin_rounds_create3(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_mpc_weights* w,
                            const cmpc_lin_rounds_dims* dims, const cmpc_lin_rounds_init* in, const cmpc_opts* opts,
                            cmpc_lin_rounds** out) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!out || !prm || !w || !dims || !in) return fail(ctx, CMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const LinInit li{0, 0, 0, in->A, in->B, in->qlin_own, in->C_own, in->h_own, in->x0, in->u_prev, in->nbr, in->traj};
    return lin_create(ctx, prm, w, dims, li, false, opts, out);
}

int cmpc_lin_rounds_create_table3(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_mpc_weights* w,
                                  const cmpc_lin_rounds_dims* dims, const cmpc_lin_rounds_table_init* in,
                                  const cmpc_opts* opts, cmpc_lin_rounds** out) {
    if (!ctx) return CMPC_ERR_ARG;
    if (!out || !prm || !w || !dims || !in) return fail(ctx, CMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const LinInit li{in->T, in->mode, in->t0, in->A, in->B, in->qlin, in->C, in->h, in->x0, in->u_prev, in->nbr, in->traj};
    return lin_create(ctx, prm, w, dims, li, true, opts, out);
}

int cmpc_lin_rounds_pos_dim(cmpc_lin_rounds* h, int* pos_dim) {
    if (!h) return CMPC_ERR_ARG;
    if (!pos_dim) return fail(h->ctx, CMPC_ERR_ARG, "null output");
    *pos_dim = h->pos_dim;
    return CMPC_OK;
}

int cmpc_lin_rounds_step(cmpc_lin_rounds* h, int rounds, int* rounds_done) {
    if (!h) return CMPC_ERR_ARG;
    const cmpc_lin_dims rd{h->d.batch, h->d.N, h->d.nb, h->d.self_offset, h->md.nx, h->mo};
    if (h->T) {  // a stage table: the window at the handle's time, which a round that ran moves on
        const cmpc_lin_table_dims td{h->T, h->mode};
        const cmpc_lin_table tab{h->A_tab, h->B_tab, h->qlin_own, h->C_own, h->h_own};
        return step_rounds(h, rounds, rounds_done, "cmpc_lin_rounds_step: log event",
                           [&](const cmpc_mpc_data* din, const cmpc_mpc_out* dout, hipStream_t s) {
                               const int rc =
                                   h->pos_dim == 3
                                       ? cmpc_lin3_table_round_dev(h->ctx, &h->prm3, &rd, h->nbr, &td, &tab, h->t,
                                                                   h->traj_all, &h->md, &h->w, din, dout, &h->opts,
                                                                   h->traj_local, s)
                                       : cmpc_lin_table_round_dev(h->ctx, &h->prm, &rd, h->nbr, &td, &tab, h->t,
                                                                  h->traj_all, &h->md, &h->w, din, dout, &h->opts,
                                                                  h->traj_local, s);
                               if (rc == CMPC_OK)
                                   h->t = h->mode == CMPC_TABLE_PERIODIC ? (h->t + 1) % h->T : std::min(h->t + 1, h->T - 1);
                               return rc;
                           });
    }
    const cmpc_lin_own own{h->qlin_own, h->C_own, h->h_own};
    return step_rounds(h, rounds, rounds_done, "cmpc_lin_rounds_step: log event",
                       [&](const cmpc_mpc_data* din, const cmpc_mpc_out* dout, hipStream_t s) {
                           return h->pos_dim == 3
                                      ? cmpc_lin3_round_dev(h->ctx, &h->prm3, &rd, h->nbr, &own, h->traj_all, &h->md,
                                                            &h->w, din, dout, &h->opts, h->traj_local, s)
                                      : cmpc_lin_round_dev(h->ctx, &h->prm, &rd, h->nbr, &own, h->traj_all, &h->md,
                                                           &h->w, din, dout, &h->opts, h->traj_local, s);
                       });
}

// ---- consensus steps (include/cmpc.h, cmpc_lin_rounds_step_consensus) ----

// One consensus step: inner rounds of build, solve, publish and exchange at the handle's state and time until the
// stopping rule (cmpc.scenarios.consensus_stop) ends them, then the advance.  *inner: the inner rounds of a step
// that was counted (0: it was not).  Returns at the first error; the caller synchronises.
static int consensus_step(cmpc_lin_rounds* h, const cmpc_consensus_opts& co, hipStream_t s, int* inner) {
    cmpc_ctx* ctx = h->ctx;
    *inner = 0;
    const bool lpt = h->d.flags & CMPC_ROUNDS_LPT, p3 = h->pos_dim == 3;  // p3: the cmpc_lin3_* entries
    const int round = h->rounds_done;
    const size_t slot = (size_t)(round % h->history) * h->d.batch;  // this step's row of the history ring
    const cmpc_mpc_data din{h->A, h->B, h->x0, h->u_prev, h->qlin, h->C, h->h};
    const cmpc_mpc_out dout{h->z, h->kkt + slot, h->iters + slot, h->status + slot};
    const cmpc_lin_dims rd{h->d.batch, h->d.N, h->d.nb, h->d.self_offset, h->md.nx, h->mo};
    const cmpc_lin_own own{h->qlin_own, h->C_own, h->h_own};
    const cmpc_lin_table_dims td{h->T, h->mode};
    const cmpc_lin_table tab{h->A_tab, h->B_tab, h->qlin_own, h->C_own, h->h_own};
    int rc;
    if ((rc = reselect(h, s)) != CMPC_OK) return rc;
    HIP_TRY(log_mark(h->log, round, 0, s));
    ConsensusLoop loop{co};
    int j = 0;
    for (;;) {
        ++j;
        if (p3)
            rc = h->T ? cmpc_lin3_table_build_dev(ctx, &h->prm3, &rd, h->md.nu, &td, &tab, h->t, h->nbr, h->traj_all,
                                                  h->A, h->B, h->qlin, h->C, h->h, s)
                      : cmpc_lin3_build_dev(ctx, &h->prm3, &rd, h->nbr, &own, h->traj_all, h->qlin, h->C, h->h, s);
        else
            rc = h->T ? cmpc_lin_table_build_dev(ctx, &h->prm, &rd, h->md.nu, &td, &tab, h->t, h->nbr, h->traj_all,
                                                 h->A, h->B, h->qlin, h->C, h->h, s)
                      : cmpc_lin_build_dev(ctx, &h->prm, &rd, h->nbr, &own, h->traj_all, h->qlin, h->C, h->h, s);
        h->opts.order = (lpt && (round > 0 || j > 1)) ? h->order : nullptr;
        if (rc == CMPC_OK) rc = cmpc_solve_mpc_batch_dev(ctx, &h->md, &h->w, &din, &dout, &h->opts, s);
        if (rc != CMPC_OK) {
            log_abandon(h->log, round);
            return rc;
        }
        // the next solve's launch order, stream-ordered after this one
        if (lpt && (rc = cmpc_order_by_iters_dev(ctx, h->d.batch, h->iters + slot, h->order, s)) != CMPC_OK) return rc;
        HIP_TRY(hipMemsetAsync(h->counts, 0, sizeof(int), s));
        rc = p3 ? cmpc_lin3_publish_dev(ctx, &h->prm3, &rd, h->md.ns, h->md.nu, h->z, h->traj_all, co.atol, co.rtol,
                                        h->traj_local, h->close, h->delta, h->counts, s)
                : cmpc_lin_publish_dev(ctx, &h->prm, &rd, h->md.ns, h->md.nu, h->z, h->traj_all, co.atol, co.rtol,
                                       h->traj_local, h->close, h->delta, h->counts, s);
        if (rc != CMPC_OK) return rc;
        if ((rc = exchange(h, s)) != CMPC_OK) return rc;
        // the node's count, not this rank's: every rank must leave the loop after the same inner round (a rank
        // that left alone would keep the others waiting in the next all-gather)
        if (h->sharded() && (rc = cmpc_comm_sum_i32(ctx, h->counts, 1, s)) != CMPC_OK) return rc;
        int count = 0;
        HIP_TRY(hipMemcpyAsync(&count, h->counts, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (loop.after(count)) break;
    }
    HIP_TRY(log_mark(h->log, round, 1, s));
    // x0, u_prev from the final z; traj_local again, with the values the last inner round exchanged
    rc = p3 ? cmpc_lin3_advance_dev(ctx, &h->prm3, &rd, h->md.ns, h->md.nu, h->z, h->x0, h->u_prev, h->traj_local, s)
            : cmpc_lin_advance_dev(ctx, &h->prm, &rd, h->md.ns, h->md.nu, h->z, h->x0, h->u_prev, h->traj_local, s);
    if (rc != CMPC_OK) return rc;
    ++h->rounds_done;
    if (h->T) h->t = h->mode == CMPC_TABLE_PERIODIC ? (h->t + 1) % h->T : std::min(h->t + 1, h->T - 1);
    h->trace = std::move(loop.trace);
    h->agreed = loop.agreed;
    *inner = j;
    return log_round(h, round, h->z, h->kkt + slot, h->iters + slot, h->status + slot, s);
}

int cmpc_lin_rounds_step_consensus(cmpc_lin_rounds* h, int steps, const cmpc_consensus_opts* co, int* steps_done,
                                   int* inner_total) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    const cmpc_consensus_opts o = co ? *co : kConsensusDefaults;
    int done = 0, total = 0, rc;
    if ((rc = check_consensus(h, steps, o)) != CMPC_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (int i = 0; i < steps && rc == CMPC_OK; ++i) {
        int inner = 0;
        rc = consensus_step(h, o, s, &inner);
        if (inner) ++done;
        total += inner;
    }
    // one more host synchronisation, also after an error: what was queued has then finished
    const hipError_t e = hipStreamSynchronize(s);
    if (steps_done) *steps_done = done;
    if (inner_total) *inner_total = total;
    if (rc != CMPC_OK) return rc;
    HIP_TRY(e);
    return CMPC_OK;
}

int cmpc_lin_rounds_consensus_read(cmpc_lin_rounds* h, const cmpc_consensus_out* o) { return consensus_read(h, o); }

int cmpc_lin_rounds_get_time(cmpc_lin_rounds* h, int* t) {
    if (!h) return CMPC_ERR_ARG;
    if (!t) return fail(h->ctx, CMPC_ERR_ARG, "null output");
    *t = h->t;  // (0 on a fixed-window handle)
    return CMPC_OK;
}

int cmpc_lin_rounds_set_time(cmpc_lin_rounds* h, int t) {
    if (!h) return CMPC_ERR_ARG;
    if (!h->T) return fail(h->ctx, CMPC_ERR_ARG, "a fixed-window handle has no time (cmpc_lin_rounds_create_table)");
    if (t < 0 || t >= h->T) return fail(h->ctx, CMPC_ERR_ARG, "bad table time (0 <= t < T)");
    h->t = t;
    return CMPC_OK;
}

// HOST rows batch x count x ... -> rows [first_row, first_row + count) of every agent's table
int cmpc_lin_rounds_table_write(cmpc_lin_rounds* h, int first_row, int count, const cmpc_lin_table* rows) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    if (!h->T) return fail(ctx, CMPC_ERR_ARG, "a fixed-window handle has no table (cmpc_lin_rounds_create_table)");
    if (!rows) return fail(ctx, CMPC_ERR_ARG, "null argument");
    if (first_row < 0 || count < 0 || (long long)first_row + count > h->T)
        return fail(ctx, CMPC_ERR_ARG, "table rows out of range (no wrap: split a wrapped write)");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nx = h->md.nx, nu = h->md.nu, mo = h->mo;
    // one agent's `count` rows are contiguous on both sides; agents are T rows apart in the table
    auto put = [&](double* tab, const double* src, size_t per) {
        if (!src || !per || !count) return hipSuccess;
        return hipMemcpy2DAsync(tab + (size_t)first_row * per, 8 * per * h->T, src, 8 * per * count, 8 * per * count,
                                h->d.batch, hipMemcpyHostToDevice, s);
    };
    if (count && (rows->A || rows->B)) h->opts.flags &= ~CMPC_FLAG_LTI;  // the rows may differ now
    HIP_TRY(put(h->A_tab, rows->A, nx * nx));
    HIP_TRY(put(h->B_tab, rows->B, nx * nu));
    HIP_TRY(put(h->qlin_own, rows->qlin, nx));
    HIP_TRY(put(h->C_own, rows->C, mo * nx));
    HIP_TRY(put(h->h_own, rows->h, mo));
    HIP_TRY(hipStreamSynchronize(s));
    return CMPC_OK;
}

int cmpc_lin_rounds_read(cmpc_lin_rounds* h, const cmpc_lin_rounds_out* o) { return read_rounds(h, o); }

int cmpc_lin_rounds_history(cmpc_lin_rounds* h, int first_round, int count, double* kkt, int* iters, int* status) {
    return history_rounds(h, first_round, count, kkt, iters, status);
}

// the measured state of a real loop replaces the predicted one (HOST pointers, either may be NULL)
int cmpc_lin_rounds_set_state(cmpc_lin_rounds* h, const double* x0, const double* u_prev) {
    if (!h) return CMPC_ERR_ARG;
    cmpc_ctx* ctx = h->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t B = h->d.batch;
    if (x0) HIP_TRY(upload(h->x0, x0, 8 * B * h->md.nx, s));
    if (u_prev) HIP_TRY(upload(h->u_prev, u_prev, 8 * B * h->md.nu, s));
    HIP_TRY(hipStreamSynchronize(s));
    return CMPC_OK;
}

int cmpc_lin_rounds_get_traj(cmpc_lin_rounds* h, double* traj_local) { return get_traj(h, traj_local); }
int cmpc_lin_rounds_set_traj(cmpc_lin_rounds* h, const double* traj_all) { return set_traj(h, traj_all); }
int cmpc_lin_rounds_destroy(cmpc_lin_rounds* h) { return destroy(h); }
int cmpc_lin_rounds_log_enable(cmpc_lin_rounds* h, int capacity, int flags) {
    return h ? log_enable(h, capacity, flags, h->md.nx, h->md.nu, h->prm.ix, h->md.ns) : CMPC_ERR_ARG;
}
int cmpc_lin_rounds_log_range(cmpc_lin_rounds* h, int* first_round, int* count) { return log_range(h, first_round, count); }
int cmpc_lin_rounds_log_read(cmpc_lin_rounds* h, int first_round, int count, const cmpc_rounds_log* o) {
    return log_read(h, first_round, count, o);
}

}  // extern "C"
