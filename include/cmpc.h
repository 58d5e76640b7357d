/* cmpc.h — C ABI of the MI355X-native collaborative-MPC QP solver (libcmpc.so).
 *
 * Drop-in boundary for the reference's per-control-step distributed QP path
 * (MarcFacerias/ColaborativeMPC-; paths relative to planner/lib/plan_lib/):
 *
 *   reference call site                                  replaced by
 *   ---------------------------------------------------  ---------------------------------
 *   PlannerLPV.solve (distributedPlanner/                cmpc_solve_lpv_batch[_dev]
 *     LPV_Planner.py:115-182): _EstimateABC :477-591,     (LPV scheduling + hyperplanes +
 *     compute_hyperplane planes/compute_plane.py:41-68,   weights + QP build fused on the
 *     compute_weights utilities/misc.py:10-18, builders   GPU, then the batched condensed
 *     :251-475, osqp_solve_qp :192-249                     IPM; one call = every agent)
 *   osqp_solve_qp(P,q,G,h,A,b) (LPV_Planner.py:192-249)   cmpc_solve_mpc_batch[_dev] for the
 *     on the structured LTV QP                            structured form (any nx, nu, N)
 *   quadprog(H,f,A,b,Aeq,beq,lb,ub) reached through       cmpc_solve_qp_batch (dense
 *     YALMIP callquadprog.m:63-69                         standard form, quadprog semantics)
 *     (Matlab-tests/yalmip/.../solvers/callquadprog.m)
 *   ROS topic exchange of predicted trajectories          cmpc_allgather_trajectories (RCCL
 *     (ROS/src/planner_experiments/src/LPV_ROS_main.py     all-gather, cmpc_comm_*); the solver
 *     :66-77,124-150) / LPV_HP_N_main.py:117              reads neighbour rows from device memory
 *
 * Conventions
 *  - All floating point is IEEE fp64, row-major, batch-major (agent b's block is
 *    contiguous).  No torch / C++ types cross this boundary.
 *  - Plain entry points take HOST pointers (the library stages them through
 *    device memory); *_dev entry points take DEVICE pointers plus a hipStream_t
 *    passed as void* (0 = default stream) and never synchronise the host.
 *  - Return value: CMPC_OK (0) or a negative CMPC_ERR_* code (API error);
 *    cmpc_last_error() gives the message.  Numerical outcome is reported per
 *    problem in status[] with OSQP's status_val codes so the reference's
 *    feasibility rule (status in {1, 2, -2}, LPV_Planner.py:246-248) applies
 *    unchanged.
 *  - A context is bound to one device and is not re-entrant: one context per
 *    host thread / stream.  One process per GPU for multi-GPU.
 *  - There is no CPU fallback: without a usable gfx950 device every solve
 *    returns CMPC_ERR_DEVICE.
 */
#ifndef CMPC_H
#define CMPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define CMPC_ABI_VERSION 6   /* 2: cmpc_lpv_advance_dev status / infeasible, cmpc_lpv_rounds_*; 3: cmpc_opts.order;
                                4: cmpc_comm_sum_i32, cmpc_plan_mpc; 5: CMPC_FLAG_POLISH;
                                6: cmpc_plan_info waves_per_agent / polish_lds_bytes / polish_max_active;
                                still 6 (additions only: no struct grew, no entry point changed):
                                cmpc_nbr_select_dev, CMPC_ROUNDS_RESELECT; cmpc_order_by_iters_dev,
                                cmpc_di_rounds_*, CMPC_ROUNDS_LPT; cmpc_round_log_dev,
                                cmpc_lpv_rounds_log_* / cmpc_di_rounds_log_*, CMPC_LOG_SEPARATION;
                                cmpc_mpc_duals, cmpc_solve_mpc_batch_duals[_dev], cmpc_mpc_duals_dev;
                                CMPC_FLAG_CERTIFY, cmpc_mpc_cert, cmpc_mpc_certify[_dev];
                                CMPC_FLAG_CERTIFY_ROWS, cmpc_mpc_cert_rows, cmpc_mpc_certify_rows[_dev];
                                CMPC_FLAG_LPV, CMPC_FLAG_LPV_AUTO, cmpc_mpc_lpv_level[_dev];
                                CMPC_FLAG_LPV_SPLIT, cmpc_mpc_lpv_split_dev;
                                cmpc_lin_build_dev, cmpc_lin_advance_dev, cmpc_lin_round_dev, cmpc_lin_rounds_*;
                                CMPC_TABLE_HOLD / _PERIODIC, cmpc_lin_table_dims, cmpc_lin_table,
                                cmpc_lin_table_build_dev, cmpc_lin_table_round_dev, cmpc_lin_rounds_table_init,
                                cmpc_lin_rounds_create_table, cmpc_lin_rounds_get_time / _set_time / _table_write;
                                cmpc_lin_publish_dev, cmpc_consensus_opts, cmpc_consensus_out,
                                cmpc_lin_rounds_step_consensus, cmpc_lin_rounds_consensus_read;
                                cmpc_lpv_publish_dev, cmpc_lpv_rounds_step_consensus,
                                cmpc_lpv_rounds_consensus_read;
                                cmpc_lin3_params, cmpc_lin3_build_dev, cmpc_lin3_table_build_dev,
                                cmpc_lin3_advance_dev, cmpc_lin3_publish_dev, cmpc_lin3_round_dev,
                                cmpc_lin3_table_round_dev, cmpc_nbr_select3_dev, cmpc_lin_rounds_create3,
                                cmpc_lin_rounds_create_table3, cmpc_lin_rounds_pos_dim */

/* API error codes */
#define CMPC_OK 0
#define CMPC_ERR_ARG (-1)
#define CMPC_ERR_DEVICE (-2)
#define CMPC_ERR_UNSUPPORTED (-3)
#define CMPC_ERR_NOMEM (-4)

/* Per-problem status (OSQP status_val values, LPV_Planner.py:243-249) */
#define CMPC_SOLVED 1
#define CMPC_SOLVED_INACCURATE 2
#define CMPC_MAX_ITER_REACHED (-2)
#define CMPC_PRIMAL_INFEASIBLE (-3)
#define CMPC_UNSOLVED (-10)

/* Size limits of the one-wavefront-per-agent solver (n = N*nu condensed variables). */
#define CMPC_MAX_NX 12
#define CMPC_MAX_NU 4
#define CMPC_MAX_NS 4
#define CMPC_MAX_MC 16
#define CMPC_MAX_NCOND 64      /* condensed one-wavefront-per-agent solvers (fp64); beyond it the
                                  stage-wise Riccati solver runs any horizon whose rows fit LDS
                                  (N = 125, nb <= 4 at nx = 9) */

typedef struct cmpc_ctx cmpc_ctx;

#define CMPC_FLAG_GENERIC 1  /* force the generic (runtime-dimension) kernel */
#define CMPC_FLAG_FP32 8     /* fp32 path (BASELINE cfg5): the Riccati factorisation and Newton recursions in
                                fp32 with fp64 iterates / residuals and a per-agent fp64 finish (opts.tol
                                ~1e-6) — on the stage-wise Riccati kernel where it has an fp32 instantiation
                                (nx,nu,mc = 6,3,6), on the lane-per-agent kernel with CMPC_FLAG_LANE or where
                                only that one is instantiated (nx,nu,mc,ns = 6,3,6,3 or 4,2,6,3); other
                                dimensions: CMPC_ERR_UNSUPPORTED */
#define CMPC_FLAG_RICCATI 16 /* force the stage-wise Riccati solver (fp64; the default when N*nu > 64) */
#define CMPC_FLAG_RESCUE 32 /* condensed solves (fp64): an agent whose factorisation breaks down short of
                               1e3 tol (status CMPC_UNSOLVED) continues from its last iterate on the
                               stage-wise Riccati solver (double-double near the solution) in a second
                               launch; a third launch restarts cold the rare one that fails again */
#define CMPC_FLAG_FINISH 64 /* with CMPC_FLAG_RESCUE: a breakdown whose best iterate already meets 1e3 tol
                               (status 2) is continued too, to full tolerance (slower; fewer status 2) */
#define CMPC_FLAG_LANE 128  /* lane-per-agent stage-wise solver in fp64 (one lane per agent, 64 agents per
                               wavefront: large batches of long horizons); CMPC_ERR_UNSUPPORTED for
                               dimensions it is not instantiated for (see CMPC_FLAG_FP32) */
#define CMPC_FLAG_POLISH 256 /* with CMPC_FLAG_RESCUE: OSQP's polish=True (LPV_Planner.py:233) for the interior-
                               point iterate — a condensed breakdown at the rounding floor (status 2) takes
                               its active set {lambda_r > t_r} as exact, solves that equality-constrained QP
                               (range-space KKT, two active-set corrections) and returns it when its merit
                               is lower (status 1 below tol) */
#define CMPC_FLAG_ONE_WAVE 512  /* the condensed kernel's fused double-integrator instantiation: one wavefront per
                                   agent (the default there); the stage-wise Riccati kernel: one wavefront per agent
                                   also where its latency mode (four per agent) would apply */
#define CMPC_FLAG_TWO_WAVES 1024 /* ... two wavefronts per agent (a 128-lane workgroup: split K build, the
                                   predictor's right-hand side on the second wave); bit-identical results, no
                                   faster at 512 agents on one MI355X, so opt-in.  Applies to the
                                   fused double-integrator round only (cmpc_di_solve_dev, the DS instantiation);
                                   other solves run one wavefront per agent.  Setting both wave flags is
                                   CMPC_ERR_ARG */
#define CMPC_FLAG_LTI 2048 /* the caller's promise that every agent of the batch is time-invariant: A_k and B_k are
                              bit-equal to A_0 and B_0 at every stage (-0.0 is not +0.0), and all are finite.  The
                              library may then read stage 0 only.  It never checks the promise against device
                              memory; a batch that breaks it is solved with stage 0's model.  Used by the fused
                              double-integrator round's one-wave instantiation (cmpc_di_solve_dev /
                              cmpc_di_round_dev: the condensed dynamics are tabulated once per solve instead of
                              recomputed in every iteration, bit-identical results); ignored everywhere else.
                              cmpc_di_rounds_create sets it itself when the host arrays it is given pass the test */
#define CMPC_FLAG_CERTIFY 4096 /* after the solve and every rescue / polish launch, the infeasibility certificate
                                  (cmpc_mpc_certify_dev below, one more launch) runs on the agents whose status is not
                                  1 or 2: an agent with a verified Farkas ray gets status CMPC_PRIMAL_INFEASIBLE (OSQP's
                                  -3; the reference's loop quits on it, LPV_Planner.py:243-249).  z, kkt, iters of every
                                  agent and the status of every uncertified agent are bit-identical to the call without
                                  the flag (the kernel reads problem data and status only), behind every solver path.
                                  Honoured by cmpc_solve_mpc_batch[_dev], cmpc_solve_mpc_batch_duals[_dev],
                                  cmpc_solve_lpv_batch[_dev] (on the builder's rows) and so by both round handles:
                                  cmpc_lpv_rounds_step halts on -3 as on any infeasible status.  Ignored where the
                                  fused double-integrator round keeps its rows in LDS only (cmpc_di_solve_dev /
                                  cmpc_di_round_dev on a v3 instantiation: no rows in memory to certify against, as for
                                  CMPC_FLAG_POLISH there) and when out->status is NULL */
#define CMPC_FLAG_CERTIFY_ROWS 8192 /* with CMPC_FLAG_CERTIFY (alone: CMPC_ERR_ARG): after the single-row launch, the
                                       combined-row certificate (cmpc_mpc_certify_rows_dev below, one more launch,
                                       CMPC_CERT_ROWS_MAX_ITER / CMPC_CERT_ROWS_CHECK_EVERY) runs on the agents whose
                                       status is still not 1, 2 or -3: hard rows that are each reachable alone but
                                       contradict each other.  Same conditions, same guarantee: z, kkt, iters of
                                       every agent and the status of every uncertified agent are bit-identical to
                                       the call without the flag.  A horizon whose iterates do not fit the
                                       certificate's LDS (cmpc_mpc_certify_rows) keeps the single-row statuses */
#define CMPC_FLAG_LPV 16384 /* the caller's promise that every agent of the batch conforms to the reference structure
                                (cmpc_mpc_lpv_level below: level 1 or 2).  On an eligible batch the specialised
                                condensed kernel then runs its compact instantiation (the one cmpc_solve_lpv_batch
                                runs: about half the LDS image, cmpc_plan_mpc reports it); on any other batch the flag
                                is ignored.  The library never checks the promise against device memory: a batch that
                                breaks it is solved as if every entry outside the pattern held the pattern's value
                                (memory-safe: the compact loads stay inside the same arrays).  Everything behind the
                                solve (rescue, polish, duals, both certificates) reads the caller's arrays as before.
                                Honoured by cmpc_solve_mpc_batch[_dev] and cmpc_solve_mpc_batch_duals[_dev]; ignored by
                                the round handles and the fused double-integrator round */
#define CMPC_FLAG_LPV_AUTO 32768 /* HOST-pointer entries only (cmpc_solve_mpc_batch, cmpc_solve_mpc_batch_duals): after
                                    the upload the detector (cmpc_mpc_lpv_level_dev) runs on the device copies and the
                                    library reads its nonconforming count back (4 bytes, one stream wait); the call
                                    then behaves as with CMPC_FLAG_LPV when the count is 0 and as with neither flag
                                    otherwise.  On cmpc_solve_mpc_batch_dev / _duals_dev: CMPC_ERR_ARG (it would need a
                                    host wait and could not be captured).  With CMPC_FLAG_LPV as well: CMPC_FLAG_LPV.
                                    Ignored where CMPC_FLAG_LPV is */
#define CMPC_FLAG_LPV_SPLIT 65536 /* the per-agent form of CMPC_FLAG_LPV_AUTO, decided on the device on every call: on an
                                     eligible batch (cmpc_mpc_lpv_level below) the single condensed launch becomes four
                                     on the same stream: the detector into a per-agent level, the partition
                                     (cmpc_mpc_lpv_split_dev below), the compact instantiation on the conforming agents
                                     and the general one on the others (both with one workgroup per agent of the batch:
                                     a workgroup beyond its list's count returns at once).  Nothing comes back to the
                                     host and nothing is promised: an agent off the pattern is solved from all of its
                                     data.  Rescue, polish, duals and both certificates follow unchanged on the whole
                                     batch.  Guarantee: per agent, z, kkt, iters, status (and y, dua_res of the duals
                                     entries) are bit-identical to a reference call on the same batch and options: for a
                                     conforming agent the call with CMPC_FLAG_LPV, for any other agent the call with no
                                     structure flag.  Scratch: 3 batch + 2 ints of the context's arena.  Honoured by
                                     cmpc_solve_mpc_batch[_dev] and cmpc_solve_mpc_batch_duals[_dev] (stream-ordered
                                     on the device entries: no host wait).  With CMPC_FLAG_LPV as well the promise wins
                                     (no detection); with CMPC_FLAG_LPV_AUTO on a host entry this flag decides (on a
                                     device entry CMPC_FLAG_LPV_AUTO stays CMPC_ERR_ARG).  Ignored on a batch that is
                                     not eligible and wherever CMPC_FLAG_LPV is ignored.  cmpc_plan_mpc accepts it and
                                     reports what it reports without it: the general image, the worst case over the
                                     two launches */
#define CMPC_FLAG_ALL (CMPC_FLAG_GENERIC | CMPC_FLAG_FP32 | CMPC_FLAG_RICCATI | CMPC_FLAG_RESCUE | CMPC_FLAG_FINISH | \
                       CMPC_FLAG_LANE | CMPC_FLAG_POLISH | CMPC_FLAG_ONE_WAVE | CMPC_FLAG_TWO_WAVES | CMPC_FLAG_LTI | \
                       CMPC_FLAG_CERTIFY | CMPC_FLAG_CERTIFY_ROWS | CMPC_FLAG_LPV | CMPC_FLAG_LPV_AUTO | \
                       CMPC_FLAG_LPV_SPLIT)
                       /* other bits: CMPC_ERR_ARG */

typedef struct {
    double tol;    /* relative stationarity/feasibility tolerance (complementarity: 1e-4*tol); <= 0 selects 1e-9 */
    int max_iter;  /* interior-point iteration cap; <= 0 selects 60 */
    int flags;     /* CMPC_FLAG_* */
    void* stamps;  /* optional DEVICE buffer, batch x 16 uint64: per-section shader-clock counts of the
                      specialised kernel (diagnostic; NULL in production) */
    const int* order; /* optional DEVICE array, batch int32, a permutation of 0..batch-1: the launch order of
                         the stage-wise Riccati solver (workgroup i solves agent order[i]; every output stays
                         at its agent's index).  With many agents per SIMD the launch ends with its slowest
                         solves; listing last round's agents by descending IPM iterations starts them first
                         (cmpc.rounds.DIRounds(lpt=True)).  The lane-per-agent solver (CMPC_FLAG_FP32 /
                         LANE) packs its wavefronts in this order, so each holds agents of similar
                         iteration counts.  Honoured by cmpc_solve_mpc_batch_dev; NULL:
                         identity.  Entries are clamped into range.  A non-permutation is undefined
                         behaviour: a missing agent is left unsolved, and a duplicated one is solved by
                         two workgroups (lanes) at once into the same scratch and outputs (a data race).
                         The library does not check it (the device array is read by the kernels only);
                         cmpc.rounds.DIRounds builds it by argsort, always a permutation.
                         Exception: a lane-per-agent batch whose scratch reaches 2 GiB runs as consecutive
                         sub-launches in agent order (mpc_lane.hip) and ignores both `order` and `stamps`
                         (same results; only the wavefront packing is lost).  cfg5 (8192 agents) stays
                         below that size; the bound is ~19.7k agents at N = 50. */
} cmpc_opts;

int cmpc_abi_version(void);
/* Create a context on HIP device `device` (ordinal among visible devices). */
int cmpc_create(cmpc_ctx** ctx, int device);
int cmpc_destroy(cmpc_ctx* ctx);
const char* cmpc_last_error(const cmpc_ctx* ctx);

/* ------------------------------------------------------------------------
 * Structured LTV agent-QP batch (the hot path).  For every agent b:
 *
 *   z = [xi_0 .. xi_N | u_0 .. u_{N-1} | du_0 .. du_{N-1}],  xi_k = [x_k (nx) | s_k (ns)]
 *   min  1/2 z'Pz + q'z  with  P = 2 blkdiag((Q (+) diag(Qs))^(N+1), R^N, dR^N),
 *                              q = 2 [qlin_0 .. qlin_N (state part), 0, 0]
 *   s.t. x_0 = x0,  x_{k+1} = A_k x_k + B_k u_k,  du_0 = u_0 - u_prev,  du_k = u_k - u_{k-1}
 *        C_{k,r} . x_k + sign_r * s_k[slack_r] <= h_{k,r}   (k = 1..N, r < mc; slack_r = -1: none)
 *        u_lb <= u_k <= u_ub   (rows ordered [u_i <= ub_i; -u_i <= -lb_i] per input, per stage)
 *
 * which is exactly the reference-form QP of PlannerLPV (LPV_Planner.py:279-475) for
 * nx=9, ns=3, nu=2 (cost :382-427, equalities :429-475, rows :251-380).  Rows with an
 * infinite bound are inactive.  Solved in condensed form (x eliminated; H = G'WG built
 * on MFMA) by a Mehrotra interior-point method, one wavefront per agent.
 * ---------------------------------------------------------------------- */
typedef struct {
    int nx, nu, N, ns, mc; /* state, input, horizon, slacks per stage, state rows per stage */
    int batch;             /* number of agents */
} cmpc_mpc_dims;

typedef struct { /* batch-shared (always HOST pointers; copied into the launch) */
    const double* Q;      /* nx*nx */
    const double* R;      /* nu*nu */
    const double* dR;     /* nu*nu */
    const double* Qs;     /* ns (diagonal slack weights, > 0) */
    const double* u_ub;   /* nu (+inf allowed) */
    const double* u_lb;   /* nu (-inf allowed) */
    const int* row_slack; /* mc: slack index used by row r, or -1 */
    const int* row_sign;  /* mc: +1 / -1 coefficient of that slack */
} cmpc_mpc_weights;

typedef struct { /* per-agent, batch-major */
    const double* A;      /* batch x N x nx x nx */
    const double* B;      /* batch x N x nx x nu */
    const double* x0;     /* batch x nx */
    const double* u_prev; /* batch x nu */
    const double* qlin;   /* batch x (N+1) x nx */
    const double* C;      /* batch x N x mc x nx   (stage k = 1..N) */
    const double* h;      /* batch x N x mc */
} cmpc_mpc_data;

typedef struct {
    double* z;    /* batch x nz,  nz = (nx+ns)(N+1) + 2 nu N  (reference layout) */
    double* kkt;  /* batch: final scaled KKT residual (may be NULL) */
    int* iters;   /* batch (may be NULL) */
    int* status;  /* batch: CMPC_SOLVED ... (may be NULL) */
} cmpc_mpc_out;

int cmpc_solve_mpc_batch(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                         const cmpc_mpc_data* host_in, const cmpc_mpc_out* host_out,
                         const cmpc_opts* opts);
int cmpc_solve_mpc_batch_dev(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                             const cmpc_mpc_data* dev_in, const cmpc_mpc_out* dev_out,
                             const cmpc_opts* opts, void* hip_stream);

/* The dual solution of the same QP in OSQP's form (the reference's res.y).  With the inequalities G z <= h in
 * the order above (the stage rows k = 1..N, r < mc, then per stage and input [u_i <= ub_i; -u_i <= -lb_i]:
 * m = N mc + 2 nu N rows) and the equalities A z = b ((nx+ns)(N+1) rows: x_0 = x0, the dynamics, an empty
 * 0 = 0 row per slack; then nu N input-rate rows), OSQP stacks [G; A]:
 *
 *   y = [y_G (m) | y_A ((nx+ns)(N+1) + nu N)],   stationarity  P z + q + G'y_G + A'y_A = 0.
 *
 * y_G is the interior-point multiplier lambda >= 0 of the iterate returned in z; a row whose bound is infinite
 * has y exactly 0.  y_A follows from z and y_G:
 *   input-rate rows   nu_d,0 = 2 dR du_0,  nu_d,i = -2 dR du_i  (i >= 1)
 *   state rows        g_k = 2 Q x_k + 2 qlin_k + C_k' lambda_k  (the last term for k >= 1)
 *                     nu_N = -g_N,  nu_k = A_k' nu_{k+1} - g_k  (k = N-1 .. 0)     (the costates)
 *   slack rows        exactly 0
 * so the x and du columns of the stationarity vector vanish by construction and the u and slack columns carry
 * the dual residual; dua_res = ||P z + q + [G; A]'y||_inf, unscaled (OSQP's info.dua_res).
 *
 * An agent whose exit does not hold the multipliers of the iterate it returns (a stall, iteration-cap or
 * breakdown exit short of tolerance restores its best iterate) and an agent whose z is not finite get an
 * all-NaN y row and a NaN dua_res.  A solve that ends at CMPC_SOLVED always has its dual solution; so does
 * every point the polish (CMPC_FLAG_POLISH) returns: max(lambda_A, 0) on its active set, 0 elsewhere.
 * z, kkt, iters and status are bit-identical to cmpc_solve_mpc_batch[_dev] with the same options.
 * CMPC_FLAG_FP32 and CMPC_FLAG_LANE: CMPC_ERR_UNSUPPORTED.  A NULL duals or duals->y: CMPC_ERR_ARG; batch == 0:
 * CMPC_OK without a launch. */
typedef struct {
    double* y;        /* batch x (m + (nx+ns)(N+1) + nu N), OSQP order [G rows; A rows] */
    double* dua_res;  /* batch (may be NULL) */
} cmpc_mpc_duals;

int cmpc_solve_mpc_batch_duals(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                               const cmpc_mpc_data* host_in, const cmpc_mpc_out* host_out,
                               const cmpc_mpc_duals* host_duals, const cmpc_opts* opts);
int cmpc_solve_mpc_batch_duals_dev(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                                   const cmpc_mpc_data* dev_in, const cmpc_mpc_out* dev_out,
                                   const cmpc_mpc_duals* dev_duals, const cmpc_opts* opts, void* hip_stream);
/* The dual kernel alone (one launch, graph-capturable): z = batch x nz and lam = batch x m inequality
 * multipliers in G's row order, both on the device; of dev_in it reads A, B, qlin, C and h.  An agent with a
 * non-finite z gets the NaN row; a NaN in lam at a finite-bound row propagates into that agent's outputs. */
int cmpc_mpc_duals_dev(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                       const cmpc_mpc_data* dev_in, const double* z, const double* lam,
                       const cmpc_mpc_duals* dev_duals, void* hip_stream);

/* Primal-infeasibility certificate of the same QP: OSQP's status -3 with its res.prim_inf_cert, for the structured
 * solves.  -3 is only ever reported with a ray that has been verified, never on a heuristic.
 *
 * Single-row reachability.  A hard stage row (k, r), k = 1..N, with row_slack[r] == -1 and finite h_{k,r}, asks
 * c'x_k <= h with c = C_{k,r}.  The adjoint recursion p_k = c, g_j = B_j' p_{j+1}, p_j = A_j' p_{j+1} (j = k-1 .. 0)
 * gives c'x_k = p_0'x0 + sum_j g_j'u_j, so the smallest value the row can take over the input box is
 *   reach = p_0'x0 + sum_{j<k, i} min(g_ji lb_i, g_ji ub_i)
 * (a term with g_ji == 0 counts 0; a term whose minimising bound is infinite disqualifies the row).  With
 *   S = |h| + sum_s |p_0s x0_s| + sum_{j,i} |g_ji| |the minimising bound|
 * the QP is infeasible when reach - h > CMPC_CERT_TOL * S.  The rounding of these sums is bounded by about
 * (k nx + N nu) 2^-53 S, at most 2e-13 S at the library's largest sizes, so 1e-9 leaves three orders of margin.
 * Among an agent's candidate rows the largest (reach - h) / S wins, ties to the smallest k, then r; a candidate
 * with a non-finite ratio (NaN or infinite data) is no candidate.  u_lb_i > u_ub_i for any input: no certificate
 * is attempted.
 *
 * The Farkas ray in the layout of cmpc_mpc_duals.y ([y_G | y_A], ny = m + (nx+ns)(N+1) + nu N):
 *   y_G   1 at row (k, r); for j < k and input i, t = -g_ji: t on the u_i <= ub_i row when t > 0, -t on the
 *         -u_i <= -lb_i row when t < 0; 0 elsewhere
 *   y_A   nu_j = -p_j on the state rows j <= k, 0 beyond; 0 on the slack rows and the input-rate rows
 * so that G'y_G + A'y_A = 0 and h'y_G + b'y_A = -(reach - h) < 0 by construction.
 *
 * The certificate is sufficient, not necessary: infeasibility that needs two or more rows combined (or a soft
 * row, which a slack always satisfies) gets no certificate from this rule, and such an agent's status stays what
 * the solver gave; the combined-row certificate below (cmpc_mpc_cert_rows) covers several hard rows combined.  Out
 * of scope: rays from the solver's diverging multipliers; a pre-solve screen that spares infeasible agents their
 * iterations (it would change iters); the MEX gateways.
 *
 * cmpc_mpc_certify_dev: DEVICE pointers, one launch, graph-capturable, one wavefront per agent; of dev_in it reads
 * A, B, x0, C and h.  status (in-out, may be NULL): an agent at CMPC_SOLVED or CMPC_SOLVED_INACCURATE is skipped
 * (none of its outputs is written); a certified agent's status becomes CMPC_PRIMAL_INFEASIBLE; NULL: every agent
 * is examined.  For an examined agent: margin = the best candidate's (reach - h) / S, NaN without a candidate;
 * row = (k-1) mc + r when certified, else -1; the ray row as above when certified, else all NaN.
 * cmpc_mpc_certify: the same with HOST pointers (status, ray, margin, row are copied in and out, so a skipped
 * agent keeps what the caller put there).
 * CMPC_ERR_ARG: NULL dims, w or in, or status and cert both NULL; dimension checks as cmpc_solve_mpc_batch.
 * batch == 0: CMPC_OK without a launch. */
#define CMPC_CERT_TOL 1e-9
typedef struct {
    double* ray;     /* batch x ny, may be NULL */
    double* margin;  /* batch, may be NULL */
    int* row;        /* batch, may be NULL */
} cmpc_mpc_cert;

int cmpc_mpc_certify(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                     const cmpc_mpc_data* host_in, int* status, const cmpc_mpc_cert* host_cert);
int cmpc_mpc_certify_dev(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                         const cmpc_mpc_data* dev_in, int* status, const cmpc_mpc_cert* dev_cert, void* hip_stream);

/* Combined-row certificate: primal infeasibility that needs several hard rows combined (a hard corridor
 * c'x_k <= h1, -c'x_k <= -h2 with h2 > h1; two hard planes pinching), each row reachable alone.  As above, -3 is only
 * ever reported with a ray the library has verified; an iteration only proposes the row weights.
 *
 * H is the set of hard stage rows (row_slack[r] == -1) of finite h.  No candidate (NaN margin, 0 iterations) when H
 * is empty or u_lb_i > u_ub_i for any input.  H, the dynamics and the input box are infeasible together exactly when
 * the least-squares violation  min over the box of 1/2 ||(C x(u) - h)_+||^2  is positive, and at its minimiser the
 * violation vector is a Farkas ray.
 *   Step size   Lf = sum over (k, r) in H of sum_{j<k, i} g_ji^2, g that row's adjoint coefficients above: the
 *               squared Frobenius norm of u -> (row values), an upper bound of its Lipschitz constant.  Not finite
 *               or not > 0: no candidate.
 *   Iteration   FISTA, no restart, no line search.  u = clip(0, lb, ub), y = u, t = 1; for it = 1 .. max_iter:
 *               x forward from x0 with the inputs y; v = max(C x - h, 0) on H; backwards P <- P + C_k' v_k,
 *               g_j = B_j' P, P <- A_j' P; u+ = clip(y - g (1 / Lf), lb, ub); t+ = (1 + sqrt(1 + 4 t^2)) / 2;
 *               y = u+ + ((t - 1) / t+)(u+ - u).
 *   Check       when it % check_every == 0 and at it == max_iter: w = max(C x(u) - h, 0) on H at u (not y).
 *               max w == 0: u satisfies every hard row; stop, no certificate, margin 0 (NaN data: stop, margin NaN).
 *               Else w <- w / max w and the aggregated adjoint P_N = C_N' w_N, P_j = C_j' w_j + A_j' P_{j+1}
 *               (1 <= j < N), P_0 = A_0' P_1, g_j = B_j' P_{j+1} gives
 *                 reach = P_0'x0 + sum min(g_ji lb_i, g_ji ub_i)   (g_ji == 0 counts 0)
 *                 S     = sum |w h| + sum_s |P_0s x0_s| + sum |g_ji| |the minimising bound|,   d = reach - w'h
 *               and the agent is certified, and the iteration stops, when d > CMPC_CERT_TOL * S.  An input with an
 *               infinite bound that the aggregate touches (g_ji != 0 with an infinite minimising bound) disqualifies
 *               the check (NaN margin).
 * The check is the single-row test on the aggregated row, rigorous whatever the iteration has or has not converged
 * to.  The ray, in the layout of cmpc_mpc_duals.y: w on the stage rows; t = -g_ji split by sign onto input i's two
 * box rows of stage j, as above; nu_j = -P_j on the state rows; 0 on the slack and input-rate rows.
 *
 * The certificate is sufficient, not necessary, and is for infeasibility by a margin: the iterations needed grow
 * roughly as 1 / gap (on the test shapes a planted gap of 0.3 takes 8 .. 320 iterations, 0.01 up to about 1150, and
 * 1e-4 is often not certified within 2000), so a barely infeasible agent keeps the solver's status.  Soft rows never
 * count: a slack always satisfies them.
 *
 * cmpc_mpc_certify_rows_dev: DEVICE pointers, one launch, graph-capturable, one wavefront per agent; of dev_in it
 * reads A, B, x0, C and h.  status (in-out, may be NULL: every agent is examined): an agent at CMPC_SOLVED,
 * CMPC_SOLVED_INACCURATE or CMPC_PRIMAL_INFEASIBLE is skipped (none of its outputs is written); a certified agent's
 * status becomes CMPC_PRIMAL_INFEASIBLE.  For an examined agent: margin = d / S of the last check, NaN without a
 * candidate; iters = iterations done; nrows = rows with w > 0 at the last check; the ray row as above when
 * certified, else all NaN.  max_iter <= 0 / check_every <= 0 select CMPC_CERT_ROWS_MAX_ITER /
 * CMPC_CERT_ROWS_CHECK_EVERY.  cmpc_mpc_certify_rows: the same with HOST pointers (outputs copied in and out).
 * Argument checks as cmpc_mpc_certify; CMPC_ERR_UNSUPPORTED when the iterates of the horizon do not fit LDS
 * (8 (2 nu + mc) N bytes > 160 KB).  batch == 0: CMPC_OK without a launch. */
#define CMPC_CERT_ROWS_MAX_ITER 512
#define CMPC_CERT_ROWS_CHECK_EVERY 8
typedef struct {
    double* ray;     /* batch x ny, may be NULL */
    double* margin;  /* batch, may be NULL */
    int* iters;      /* batch, may be NULL */
    int* nrows;      /* batch, may be NULL */
} cmpc_mpc_cert_rows;

int cmpc_mpc_certify_rows(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                          const cmpc_mpc_data* host_in, int* status, const cmpc_mpc_cert_rows* host_cert,
                          int max_iter, int check_every);
int cmpc_mpc_certify_rows_dev(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                              const cmpc_mpc_data* dev_in, int* status, const cmpc_mpc_cert_rows* dev_cert,
                              int max_iter, int check_every, void* hip_stream);

/* Reference structure of a structured batch: the pattern of the reference's own agent QPs (LPV_Planner.py:493-585,
 * :279-380) under which the specialised condensed kernel keeps compact images (CMPC_FLAG_LPV).  This is the one
 * definition; cmpc.structure.lpv_level is its numpy statement, and the entries it constrains are exactly those the
 * compact (LS) load of mpc_ipm3.hip never reads (checked against that code: D_k = A_k - I on columns 0..2, B_k rows
 * 0..2, the rows' coefficients on vx / ey / (X, Y)).
 *
 * A batch is eligible when nx = 9, nu = 2, ns = 3, mc = 4 + nb with 0 <= nb <= 3, N <= 32 and N nu <= 64; row_slack is
 * {-1, 0, 1, 1, 2, ...} and row_sign {+1, +1, +1, +1, -1, ...} (a sign >= 0 counts as +1, as everywhere in the library);
 * Q has no nonzero off-diagonal entry; and none of CMPC_FLAG_GENERIC, RICCATI, LANE, FP32 is set.
 * Agent b of an eligible batch conforms when at every stage k, comparing by value (x != 0.0: -0.0 conforms, NaN does
 * not; denormals are not flushed):
 *   A[b,k,r,t] == (r == t ? 1 : 0) for every column t >= 3;   B[b,k,r,:] == 0 for every row r >= 3;
 *   C[b,k,0..1,:] is zero outside column 0, C[b,k,2..3,:] outside column 3, C[b,k,4+j,:] outside columns 7, 8.
 * Level of an agent: 0 when the batch is not eligible or the agent does not conform; else 2 when Q[1,1], Q[2,2], Q[5,5]
 * and Q[6,6] are all 0.0 (the kernel's further contraction, the reference's config_LPV.py:7), else 1.
 *
 * cmpc_mpc_lpv_level_dev: DEVICE pointers, stream-ordered, graph-capturable, no scratch: one launch (a workgroup per
 * agent streams that agent's A, B and C once) writes level[b] (may be NULL) and, after the library has zeroed it on the
 * stream, adds the number of agents at level 0 to *nonconforming (may be NULL; a device int).  A batch that is not
 * eligible gets level 0 everywhere and *nonconforming = batch without a launch (the entry takes no
 * options, so eligibility is judged with no flag set).
 * cmpc_mpc_lpv_level: the same with HOST pointers (upload, one launch, copy back; synchronises).
 * CMPC_ERR_ARG: NULL dims, w, in, in->A, in->B, NULL in->C when mc > 0, or level and nonconforming both NULL; dimension
 * errors as cmpc_solve_mpc_batch.  batch == 0: CMPC_OK without a launch. */
int cmpc_mpc_lpv_level_dev(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                           const cmpc_mpc_data* dev_in, int* level, int* nonconforming, void* hip_stream);
int cmpc_mpc_lpv_level(cmpc_ctx* ctx, const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w,
                       const cmpc_mpc_data* host_in, int* level, int* nonconforming);

/* The stable partition of a batch by the detector's level (the second launch of CMPC_FLAG_LPV_SPLIT).  DEVICE
 * pointers, one launch (one 1024-thread workgroup, 1024 agents per step), stream-ordered, no host wait, no scratch.
 * conf[0 .. nc) <- the agents with level[b] > 0 in ascending order and conf[batch] <- nc; rest[0 .. nr) <- the others
 * in ascending order and rest[batch] <- nr; nc + nr = batch.  The result is fully determined by level.  conf and rest
 * hold batch + 1 ints each; the entries conf[nc .. batch) and rest[nr .. batch) are left untouched.
 * cmpc.structure.lpv_split is its numpy statement.
 * batch == 0: CMPC_OK without a launch.  CMPC_ERR_ARG: batch < 0; a NULL pointer with batch > 0; level, conf and rest
 * overlapping each other (level over batch ints, conf and rest over batch + 1). */
int cmpc_mpc_lpv_split_dev(cmpc_ctx* ctx, int batch, const int* level, int* conf, int* rest, void* hip_stream);

/* The solver a structured batch would run, and how many of its workgroups share a CU — host only
 * (no context, no device).  Every solver uses more than 256 VGPRs + AGPRs per lane, so one
 * wavefront per SIMD (4 workgroups per CU at most); the LDS image then decides: wg_per_cu =
 * min(4, 160 KB / lds_bytes).  The lane-per-agent solver packs 32 agents per workgroup.  Errors as
 * cmpc_solve_mpc_batch (CMPC_ERR_UNSUPPORTED, CMPC_ERR_ARG). */
#define CMPC_SOLVER_CONDENSED_V3 1 /* specialised condensed kernel (mpc_ipm3: PlannerLPV row pattern) */
#define CMPC_SOLVER_CONDENSED 2    /* generic condensed kernel */
#define CMPC_SOLVER_RICCATI 3      /* stage-wise Riccati kernel (long horizons, fp32 path) */
#define CMPC_SOLVER_LANE 4         /* lane-per-agent stage-wise kernel */
typedef struct {
    int solver;        /* CMPC_SOLVER_* */
    int lds_bytes;     /* dynamic LDS per workgroup */
    int wg_per_cu;     /* workgroups resident per CU */
    int agents_per_wg; /* 1, or 32 (lane solver) */
    int waves_per_agent;   /* wavefronts of one agent's workgroup: 1; 4 for the stage-wise Riccati kernel's latency
                              mode (an LDS image over half a CU, the PlannerLPV agent at the reference's N = 125:
                              the agent's workgroup gets all four SIMDs of its CU; CMPC_FLAG_ONE_WAVE keeps one);
                              (2: the condensed kernel's CMPC_FLAG_TWO_WAVES mode of a fused double-integrator round,
                              cmpc_di_solve_dev, which the plan of a structured batch does not describe) */
    /* The rescue policy (CMPC_FLAG_RESCUE [| CMPC_FLAG_POLISH]) adds launches the fields above do not
     * describe: the polish kernel (before the Riccati hand-over and after the Riccati passes; one
     * 256-thread workgroup per agent, agents without a flag return at once) and two Riccati passes.
     * polish_lds_bytes: the polish workgroup's LDS (0 when the polish does not run); polish_max_active:
     * the largest active set it polishes (kPolishMaxActive = 96, lowered in steps of 8 until the image
     * fits 160 KB; larger active sets keep the interior-point result) */
    int polish_lds_bytes;
    int polish_max_active;
} cmpc_plan_info;
int cmpc_plan_mpc(const cmpc_mpc_dims* dims, const cmpc_mpc_weights* w, const cmpc_opts* opts,
                  cmpc_plan_info* out);

/* ------------------------------------------------------------------------
 * Reference-semantics LPV batch: one call = PlannerLPV.solve for every agent
 * (LPV_Planner.py:115-182) with the reference's exact quirks (lagged plane and
 * weight indexing, u not shifted, ey half-width from the previous prediction's s,
 * vx < 0.2 branch).  n_s = 9 states [vx vy wz ey epsi theta s X Y], 3 slacks,
 * 2 inputs [delta a].
 * ---------------------------------------------------------------------- */
#define CMPC_MAX_SEG 32

typedef struct {
    double lf, lr, m, I, Cf, Cr, mu;                   /* model_param (config/base_class.py:20-28) */
    double vx_ref, min_dist, max_vel, min_vel;         /* sys_lim (config/base_class.py:30-41) */
    double max_rs, max_ls, max_ac, max_dc;
    double dt, wq;                                     /* sample time, coverage weight */
    double Q[81], Qs[3], R[4], dR[4];                  /* gains (scripts/config_files/config_LPV.py:6-11) */
} cmpc_lpv_params;

typedef struct {     /* one lane of Map.PointAndTangent (track_initialization.py:220-300) */
    int nseg;        /* rows */
    const double* s0;         /* nseg: cumulative s at segment start (column 3) */
    const double* len;        /* nseg: segment length (column 4) */
    const double* curv;       /* nseg: signed curvature (column 5) */
    const double* half_width; /* nseg: Map.halfWidth */
} cmpc_track;

typedef struct {
    int batch, N, nb;  /* agents, horizon, neighbours per agent (same for all agents) */
    int last_rows;     /* rows of Last_xPredicted: N+1 at the first step, N afterwards */
} cmpc_lpv_dims;

typedef struct {   /* per-agent, batch-major */
    const double* x0;       /* batch x 9 */
    const double* x_last;   /* batch x last_rows x 9   (Last_xPredicted) */
    const double* u_last;   /* batch x N x 2           (uPred, not shifted) */
    const double* u_old;    /* batch x 2               ([OldSteering, OldAccelera]) */
    const double* x_agents; /* batch x (N+1) x nb x 2  (neighbour X,Y; NULL => planes 0, weights 1) */
    const double* pose;     /* batch x (N+1) x 2       (own previous X,Y) */
} cmpc_lpv_data;

typedef struct {
    double* z;       /* batch x nz (nz = 12(N+1) + 4N) */
    double* planes;  /* batch x N x 3 x nb (may be NULL) — compute_plane.py layout */
    double* kkt;     /* may be NULL */
    int* iters;      /* may be NULL */
    int* status;     /* may be NULL */
} cmpc_lpv_out;

int cmpc_solve_lpv_batch(cmpc_ctx* ctx, const cmpc_lpv_params* prm, const cmpc_track* track,
                         const cmpc_lpv_dims* dims, const cmpc_lpv_data* host_in,
                         const cmpc_lpv_out* host_out, const cmpc_opts* opts);
int cmpc_solve_lpv_batch_dev(cmpc_ctx* ctx, const cmpc_lpv_params* prm, const cmpc_track* track,
                             const cmpc_lpv_dims* dims, const cmpc_lpv_data* dev_in,
                             const cmpc_lpv_out* dev_out, const cmpc_opts* opts, void* hip_stream);

/* The LPV builder alone, DEVICE pointers: the structured agent-QP that
 * cmpc_solve_lpv_batch_dev hands its solver, for hosts that inspect or extend it before
 * cmpc_solve_mpc_batch_dev.  _EstimateABC (LPV_Planner.py:477-591: A_k = I + dt A_c, B_k = dt B_c
 * at the scheduling point of Last_xPredicted row k and uPred row k, curvature / half-width by
 * track-segment lookup misc.py:78-126), compute_hyperplane (compute_plane.py:41-68) and
 * compute_weights (misc.py:10-18) feed the rows (:251-380) and the linear cost (:382-427):
 *   A batch x N x 9 x 9, B batch x N x 9 x 2, qlin batch x (N+1) x 9, C batch x N x (4+nb) x 9,
 *   h batch x N x (4+nb), planes batch x N x 3 x nb (may be NULL), err batch (1: s of the
 *   previous prediction lies on no track segment — the reference raises there, misc.py:97). */
typedef struct {
    double *A, *B, *qlin, *C, *h, *planes;
    int* err;
} cmpc_lpv_build_out;

int cmpc_lpv_build_dev(cmpc_ctx* ctx, const cmpc_lpv_params* prm, const cmpc_track* track,
                       const cmpc_lpv_dims* dims, const cmpc_lpv_data* dev_in, const cmpc_lpv_build_out* dev_out,
                       void* hip_stream);

/* ------------------------------------------------------------------------
 * Synthetic agent family of BASELINE.json configs 1-5 (no reference counterpart:
 * the reference's model is the 9-state LPV bicycle; BASELINE fixes a double
 * integrator).  State [p (dim) | v (dim)], input a (dim), dim = 2 (nx=4, nu=2) or
 * 3 (nx=6, nu=3); 3 slacks; rows per stage mirror PlannerLPV's
 * (LPV_Planner.py:279-380) with v_x for vx, p_y - lane for ey and (p_x, p_y) for
 * (X, Y).  Per consensus round: _build rebuilds C, h, qlin of every local agent
 * from the previous round's exchanged trajectories (DEVICE pointers); _advance
 * applies the round update of LPV_HP_N_main.py:106-117 (x0 <- x_1,
 * u_prev <- u_0, trajectory <- predicted positions) and writes this rank's rows
 * of the exchange buffer.
 * ---------------------------------------------------------------------- */
typedef struct {
    int dim;                                   /* 2 or 3 */
    double v_ref, q_v, q_lane, hw, min_vel, max_vel, min_dist, wq;
} cmpc_di_params;

typedef struct {
    int batch, N, nb;   /* local agents, horizon, neighbours per agent */
    int self_offset;    /* global index of local agent 0 in traj_all */
} cmpc_di_dims;

int cmpc_di_build_dev(cmpc_ctx* ctx, const cmpc_di_params* prm, const cmpc_di_dims* dims,
                      const int* nbr /* batch x nb, global agent indices */,
                      const double* lane /* batch */,
                      const double* traj_all /* n_total x (N+1) x 2 */,
                      double* qlin /* batch x (N+1) x nx */, double* C /* batch x N x (4+nb) x nx */,
                      double* h /* batch x N x (4+nb) */, void* hip_stream);
/* Fused build + solve of one round (LPV_HP_N_main.py:96-117, build and solve of every agent):
 * where the v3 one-wave kernel covers the problem, each agent's rows and linear cost are built
 * from traj_all straight into the solver's LDS (bit-identical to cmpc_di_build_dev) — qlin / C
 * / h of `data` are then neither written nor read; otherwise this is cmpc_di_build_dev into
 * data->qlin / C / h (written despite the const) followed by cmpc_solve_mpc_batch_dev.
 * dims must describe the same agents: batch and N equal, nx = 2 dim, nu = dim, mc = 4 + nb. */
int cmpc_di_solve_dev(cmpc_ctx* ctx, const cmpc_di_params* prm, const cmpc_di_dims* ddims, const int* nbr,
                      const double* lane, const double* traj_all, const cmpc_mpc_dims* dims,
                      const cmpc_mpc_weights* w, const cmpc_mpc_data* data, const cmpc_mpc_out* out,
                      const cmpc_opts* opts, void* hip_stream);
/* cmpc_di_solve_dev followed by cmpc_di_advance_dev(z = out->z, x0 = data->x0, u_prev = data->u_prev,
 * traj_local), with the same results: where the v3 kernel covers the problem the solver's launch writes
 * x0 <- x_1, u_prev <- u_0 (data->x0 / u_prev: written despite the const) and traj_local from the
 * trajectory it holds, one launch for the round's build, solve and advance; otherwise the advance kernel
 * follows the solve.  traj_all is only read (workgroups that start later in the launch still build their
 * rows from it: the Jacobi round); the exchange traj_local -> traj_all stays the caller's next step, and
 * traj_local must not alias traj_all. */
int cmpc_di_round_dev(cmpc_ctx* ctx, const cmpc_di_params* prm, const cmpc_di_dims* ddims, const int* nbr,
                      const double* lane, const double* traj_all, const cmpc_mpc_dims* dims,
                      const cmpc_mpc_weights* w, const cmpc_mpc_data* data, const cmpc_mpc_out* out,
                      const cmpc_opts* opts, double* traj_local /* batch x (N+1) x 2 */, void* hip_stream);
int cmpc_di_advance_dev(cmpc_ctx* ctx, const cmpc_di_params* prm, const cmpc_di_dims* dims,
                        const double* z /* batch x nz */, double* x0 /* batch x nx */,
                        double* u_prev /* batch x nu */, double* traj_local /* batch x (N+1) x 2 */,
                        void* hip_stream);

/* Device-resident LPV consensus round (LPV_HP_N_main.py:96-117), DEVICE pointers, dims =
 * {batch, N, nb, self_offset} of the cmpc_di_dims struct:
 *   cmpc_lpv_gather_dev:  x_agents (batch x (N+1) x nb x 2) <- traj_all rows nbr[b][j] and pose
 *     (batch x (N+1) x 2) <- traj_all row self_offset + b — agents[:, ns[i], :] / agents[:, i, :]
 *     (:99-104); traj_all is n_total x (N+1) x 2, nbr batch x nb global agent indices;
 *   cmpc_solve_lpv_batch_dev on those buffers;
 *   cmpc_lpv_advance_dev: from z (reference layout): x0 <- xPred[1], x_last <- xPred[1:] written
 *     DENSE as batch x N x 9 (last_rows = N from the second round on, :115), u_last <- uPred
 *     (batch x N x 2, not shifted), u_old <- uPred[0] (:179-180), traj_local (batch x (N+1) x 2)
 *     <- xPred[:, X, Y] (:117); status (may be NULL) / infeasible (may be NULL, DEVICE int): the
 *     count of agents the reference calls infeasible (status not in {1, 2, -2}, LPV_Planner.py:243-249)
 *     is added to *infeasible; an agent whose z is not finite is not advanced (no NaN is exchanged);
 *   then the all-gather of traj_local into traj_all (cmpc_allgather_trajectories or torch). */
int cmpc_lpv_gather_dev(cmpc_ctx* ctx, const cmpc_di_dims* dims, const int* nbr, const double* traj_all,
                        double* x_agents, double* pose, void* hip_stream);
int cmpc_lpv_advance_dev(cmpc_ctx* ctx, const cmpc_di_dims* dims, const double* z, double* x0, double* x_last,
                         double* u_last, double* u_old, double* traj_local, const int* status, int* infeasible,
                         void* hip_stream);

/* ------------------------------------------------------------------------
 * Neighbour selection on the device, DEVICE pointers, stream-ordered, no host synchronisation.
 * The reference fixes each agent's neighbour list ns[i] once (LPV_HP_N_main.py:82-85: all other
 * agents); a population with nb < n_total - 1 whose agents overtake each other needs the list of a
 * round rebuilt from the exchange buffer every rank already holds.  For every local agent b (global
 * index g = self_offset + b) the nb nearest other agents out of the n_total trajectories of traj_all
 * (n_total x (N+1) x 2):
 *   score(g, j) = min over k in [k0, k1] of (dx dx + dy dy),  dx = traj_all[j,k,0] - traj_all[g,k,0],
 *     dy likewise, each expression rounded as written (no fma: the bits of numpy's dx*dx + dy*dy);
 *     a NaN at any stage of the window makes the score NaN (numpy's min), and a NaN score counts as +inf;
 *   window (0, 0): nearest now; (0, N): closest predicted approach;
 *   candidates are ordered by (score, j) ascending; j = g is left out by index, never by distance
 *     (an agent on the same point is a valid neighbour; g itself is never returned: the row builders
 *     divide by the distance to a neighbour);
 *   nbr[b, 0..nb) <- their global indices, nearest first; dist2[b, 0..nb) (may be NULL) <- their scores.
 * The result is fully determined by this rule, ties and non-finite coordinates included
 * (cmpc.scenarios.select_neighbours is its numpy statement).  The reference's ns[i] is in index
 * order; nearest first only reorders the collision rows of an agent's QP and the columns of `planes`.
 * CMPC_ERR_ARG: NULL dims or traj_all, or NULL nbr when batch * nb > 0; nb < 0, nb > CMPC_MAX_MC - 4 or
 * nb >= n_total; self_offset < 0 or self_offset + batch > n_total; batch < 0; N < 1; a window outside
 * 0 <= k0 <= k1 <= N.  batch == 0 or nb == 0: CMPC_OK without a launch.
 * ---------------------------------------------------------------------- */
typedef struct {
    int batch, N, nb, self_offset;   /* as cmpc_di_dims */
    int n_total;                     /* trajectories in traj_all */
    int k0, k1;                      /* stage window, 0 <= k0 <= k1 <= N */
} cmpc_nbr_dims;
int cmpc_nbr_select_dev(cmpc_ctx* ctx, const cmpc_nbr_dims* dims, const double* traj_all,
                        int* nbr /* batch x nb */, double* dist2 /* batch x nb, may be NULL */,
                        void* hip_stream);

/* ------------------------------------------------------------------------
 * The longest-first launch order of cmpc_opts.order, on the device: DEVICE pointers, stream-ordered, no
 * host synchronisation.
 *   order[0..batch) <- the agents by descending key, ties by ascending index (a stable sort):
 *     key(b) = min(max(iters[b], 0), 65535)
 * with iters the previous round's per-agent IPM iteration counts (cmpc_mpc_out.iters).  Always a
 * permutation of 0..batch-1, whatever iters holds (cmpc_opts.order requires one: a non-permutation is a
 * data race).  For keys in range it is torch.argsort(iters, descending=True, stable=True);
 * cmpc.scenarios.order_by_iters is its numpy statement.  One workgroup (a two-pass 8-bit radix sort of
 * (key, index); its launch time beside a round's solver launch: DESIGN.md section 4).  Its scratch (8 bytes
 * per agent) belongs to the context and grows on first use; a steady-state call allocates nothing.
 * order must not alias iters (CMPC_ERR_ARG).  batch == 0: CMPC_OK without a launch.  NULL pointers with
 * batch > 0, batch < 0: CMPC_ERR_ARG.
 * ---------------------------------------------------------------------- */
int cmpc_order_by_iters_dev(cmpc_ctx* ctx, int batch, const int* iters, int* order, void* hip_stream);

/* ------------------------------------------------------------------------
 * Consensus rounds behind a handle (LPV_HP_N_main.py:96-117; the one-process-per-agent ROS
 * variant ROS/src/planner_experiments/src/LPV_ROS_main.py:66-77,124-150), for hosts without
 * torch or device memory of their own (MATLAB through the MEX gateway, plain C).  The handle
 * owns every device buffer of this rank's agents and the node-global exchange buffer; a round
 * is gather -> cmpc_solve_lpv_batch_dev -> cmpc_lpv_advance_dev -> exchange, all on the
 * context's stream, so consecutive rounds never touch the host.
 *
 * Sharding: this rank holds agents [self_offset, self_offset + batch) of n_total.  The exchange
 * of a round is the identity when batch == n_total; otherwise an RCCL all-gather over the
 * context's communicator (cmpc_comm_init; ranks hold equal contiguous shards in rank order),
 * or — CMPC_ROUNDS_HOST_EXCHANGE — the host's: after cmpc_lpv_rounds_step the host reads this
 * rank's positions (cmpc_lpv_rounds_get_traj), exchanges them its own way (MPI, sockets) and
 * hands the gathered buffer back (cmpc_lpv_rounds_set_traj) before the next step.
 *
 * Failure semantics (LPV_Planner.py:243-249, LPV_HP_N_main.py:102-111): an agent is
 * infeasible when its status is not in {1, 2, -2}; the reference quits the experiment there.
 * cmpc_lpv_rounds_step counts infeasible agents per round on the device and stops after the
 * first round that has any (rounds_done < rounds).  Sharded over RCCL, the count is the
 * node's (cmpc_comm_sum_i32 over the ranks), so every rank stops in the same round; with
 * CMPC_ROUNDS_HOST_EXCHANGE (one round per step) *infeasible is this rank's count and the
 * host combines them as it exchanges positions.  An agent whose solution is not finite
 * (track lookup failed, the reference raises) keeps its previous state and trajectory, so no
 * NaN reaches a neighbour.
 * ---------------------------------------------------------------------- */
typedef struct cmpc_lpv_rounds cmpc_lpv_rounds;

#define CMPC_ROUNDS_HOST_EXCHANGE 1  /* the host exchanges positions between steps */
#define CMPC_ROUNDS_NO_HALT 2        /* run all requested rounds even after an infeasible agent */
#define CMPC_ROUNDS_RESELECT 4       /* every round starts with cmpc_nbr_select_dev, window (0, 0), on the exchange
                                        buffer as the last exchange / cmpc_lpv_rounds_set_traj left it, into the
                                        handle's neighbour table (init->nbr is then only the table's first content,
                                        replaced before it is read; needs nb < n_total).  Off: the table of
                                        init->nbr for good, as the reference */

typedef struct {
    int n_total;      /* agents over all ranks */
    int batch;        /* agents of this rank */
    int self_offset;  /* global index of this rank's agent 0 */
    int N, nb;        /* horizon, neighbours per agent */
    int flags;        /* CMPC_ROUNDS_* */
} cmpc_lpv_rounds_dims;

typedef struct {   /* HOST pointers, this rank's agents, batch-major (copied at create) */
    const double* x0;      /* batch x 9 */
    const double* x_last;  /* batch x (N+1) x 9: the first round's Last_xPredicted */
    const double* u_last;  /* batch x N x 2 */
    const double* u_old;   /* batch x 2, or NULL (zeros: PlannerLPV's initial OldSteering/OldAccelera) */
    const int* nbr;        /* batch x nb global agent indices (the reference: all other agents) */
    const double* traj;    /* n_total x (N+1) x 2 initial exchange buffer (the reference's `agents`);
                              NULL: only valid when batch == n_total, taken from x_last[:, :, 7:9] */
} cmpc_lpv_rounds_init;

typedef struct {   /* HOST pointers (any may be NULL): the latest round of this rank's agents */
    double* z;       /* batch x nz (nz = 12(N+1) + 4N) */
    double* kkt;     /* batch */
    int* iters;      /* batch */
    int* status;     /* batch */
    double* x0;      /* batch x 9: the next round's initial states */
    double* planes;  /* batch x N x 3 x nb */
} cmpc_lpv_rounds_out;

int cmpc_lpv_rounds_create(cmpc_ctx* ctx, const cmpc_lpv_params* prm, const cmpc_track* track,
                           const cmpc_lpv_rounds_dims* dims, const cmpc_lpv_rounds_init* init,
                           const cmpc_opts* opts, cmpc_lpv_rounds** out);
/* Runs up to `rounds` rounds; *rounds_done (may be NULL) receives the number completed and
 * *infeasible (may be NULL) the infeasible-agent count of the last one.  Synchronises the host. */
int cmpc_lpv_rounds_step(cmpc_lpv_rounds* h, int rounds, int* rounds_done, int* infeasible);
int cmpc_lpv_rounds_read(cmpc_lpv_rounds* h, const cmpc_lpv_rounds_out* host_out);
/* Host exchange: this rank's predicted positions (batch x (N+1) x 2) / the gathered buffer
 * (n_total x (N+1) x 2, rank order). */
int cmpc_lpv_rounds_get_traj(cmpc_lpv_rounds* h, double* traj_local);
int cmpc_lpv_rounds_set_traj(cmpc_lpv_rounds* h, const double* traj_all);
/* Destroy every handle of a context before cmpc_destroy(ctx). */
int cmpc_lpv_rounds_destroy(cmpc_lpv_rounds* h);

/* ------------------------------------------------------------------------
 * The same handle for the synthetic double-integrator family (cmpc_di_params; BASELINE cfg2-cfg5): what
 * cmpc.rounds.DIRounds.step() does with fused=True, launch for launch and bit for bit, for hosts without
 * torch or device memory of their own.  A round, on the context's stream:
 *   1. CMPC_ROUNDS_RESELECT and nb > 0: cmpc_nbr_select_dev, window (0, 0), into the handle's table;
 *   2. cmpc_di_round_dev on the handle's buffers (build, solve and advance in one launch where the v3
 *      kernel covers the problem; build, solve and advance launches elsewhere); with CMPC_ROUNDS_LPT, from
 *      the second round on, cmpc_opts.order = the handle's order buffer;
 *   3. CMPC_ROUNDS_LPT: cmpc_order_by_iters_dev of this round's iteration counts into the order buffer;
 *   4. the exchange, as cmpc_lpv_rounds_step: a device copy (one rank), the context's RCCL communicator
 *      (cmpc_allgather_trajectories), or the host's (CMPC_ROUNDS_HOST_EXCHANGE: one round per step,
 *      cmpc_di_rounds_get_traj / _set_traj in between).
 * The synthetic family has no halt rule: cmpc_di_rounds_step always runs the rounds it is asked for.
 * opts->flags go to the solver unchanged (CMPC_FLAG_FP32, the wave flags, ...); opts->stamps and
 * opts->order are ignored.  Dimension and flag combinations the solver refuses come back from the first
 * cmpc_di_rounds_step with the solver's own code and message.
 *
 * History: round r (counted from create) writes its kkt / iters / status into row r mod `history` of a
 * device ring — the solver's output pointers are set to that row, nothing is copied — so a host that calls
 * cmpc_di_rounds_step(h, 100, ...) once still gets every round's statuses and iteration counts
 * (cmpc_di_rounds_history) without one host synchronisation per round.
 *
 * CMPC_ERR_ARG at create: a NULL argument (opts may be NULL; init->nbr may be NULL when nb == 0); batch < 1,
 * self_offset < 0 or self_offset + batch > n_total; N < 1; dim not 2 or 3; nb < 0 or 4 + nb > CMPC_MAX_MC; a
 * neighbour index outside 0 <= j < n_total; CMPC_ROUNDS_RESELECT with nb >= n_total; a sharded population
 * (batch != n_total) without CMPC_ROUNDS_HOST_EXCHANGE and without a matching communicator (cmpc_comm_init:
 * equal contiguous shards in rank order); history < 0; an unknown rounds or option flag.
 * ---------------------------------------------------------------------- */
typedef struct cmpc_di_rounds cmpc_di_rounds;

#define CMPC_ROUNDS_LPT 8   /* from the second round on, cmpc_opts.order = cmpc_order_by_iters_dev of the previous
                               round's iteration counts (the first round: NULL, identity).  Only when an agent
                               runs changes, never what it returns.  cmpc_di_rounds and cmpc_lin_rounds */

typedef struct {
    int n_total, batch, self_offset;  /* as cmpc_lpv_rounds_dims */
    int N, nb;
    int flags;      /* CMPC_ROUNDS_HOST_EXCHANGE | CMPC_ROUNDS_RESELECT | CMPC_ROUNDS_LPT; CMPC_ROUNDS_NO_HALT is
                       accepted and has no effect (the synthetic family has no halt rule); other bits CMPC_ERR_ARG */
    int history;    /* rounds of per-agent kkt / iters / status kept on the device, >= 1 (0 selects 1) */
} cmpc_di_rounds_dims;

typedef struct {    /* HOST pointers, this rank's agents, copied at create: what cmpc.scenarios.make_di produces */
    const double *A, *B;        /* batch x N x nx x nx, batch x N x nx x nu   (nx = 2 dim, nu = dim) */
    const double *x0, *u_prev;  /* batch x nx, batch x nu */
    const double* lane;         /* batch */
    const int* nbr;             /* batch x nb global indices (checked: 0 <= j < n_total) */
    const double* traj;         /* n_total x (N+1) x 2 initial exchange buffer (required) */
} cmpc_di_rounds_init;

typedef struct {    /* HOST pointers, any may be NULL: the latest round of this rank's agents */
    double *z, *kkt;            /* batch x nz (nz = (nx + 3)(N+1) + 2 nu N), batch */
    int *iters, *status;        /* batch */
    double *x0, *u_prev;        /* batch x nx, batch x nu: the next round's initial state and previous input */
    int* nbr;                   /* batch x nb: the table the latest round used */
} cmpc_di_rounds_out;

/* w: ns = 3 slacks and mc = 4 + nb rows (Q nx*nx, R / dR nu*nu, Qs 3, u_ub / u_lb nu, row_slack / row_sign
 * 4 + nb), copied at create. */
int cmpc_di_rounds_create(cmpc_ctx* ctx, const cmpc_di_params* prm, const cmpc_mpc_weights* w,
                          const cmpc_di_rounds_dims* dims, const cmpc_di_rounds_init* init, const cmpc_opts* opts,
                          cmpc_di_rounds** out);
/* Runs `rounds` rounds (*rounds_done, may be NULL: the number completed); synchronises the host once, at the end. */
int cmpc_di_rounds_step(cmpc_di_rounds* h, int rounds, int* rounds_done);
int cmpc_di_rounds_read(cmpc_di_rounds* h, const cmpc_di_rounds_out* host_out);
/* Rounds [first_round, first_round + count) of the ring as count x batch arrays (any may be NULL).  A round not
 * yet run, or already overwritten (older than the last `history` rounds): CMPC_ERR_ARG. */
int cmpc_di_rounds_history(cmpc_di_rounds* h, int first_round, int count, double* kkt, int* iters, int* status);
int cmpc_di_rounds_get_traj(cmpc_di_rounds* h, double* traj_local);
int cmpc_di_rounds_set_traj(cmpc_di_rounds* h, const double* traj_all);
/* Destroy every handle of a context before cmpc_destroy(ctx). */
int cmpc_di_rounds_destroy(cmpc_di_rounds* h);

/* ------------------------------------------------------------------------
 * The experiment log of a round, on the device.  The reference's run ends in csv/<id>/{states,u,plan_dist,
 * time}.dat (config/base_class.py:64-99): per control step xPred[0], uPred[0], xPred[-1, 6] - xPred[0, 6] and the
 * solve time.  The first three are entries of the round's z.
 *
 * cmpc_round_log_dev: DEVICE pointers, stream-ordered, no host synchronisation.  One launch copies, for every
 * agent b of one round (z in the reference layout, xi_k = [x_k (nx) | s_k (ns)], nz = (nx+ns)(N+1) + 2 nu N):
 *   row->state[b, 0..nx)  <- z[b, 0 .. nx)                                      xPred[0]
 *   row->u[b, 0..nu)      <- z[b, (nx+ns)(N+1) .. +nu)                          uPred[0]
 *   row->look_ahead[b]    <- z[b, (nx+ns)N + look_col] - z[b, look_col]         one subtraction
 *   row->kkt / iters / status[b] <- kkt / iters / status[b]                     the round's solver outputs
 * bit for bit (a NaN z — an agent the builder flagged — gives NaN rows).  Any destination may be NULL: that part
 * is skipped.  The pointers are one round's rows: a caller that keeps a ring adds the row offset on the host, so
 * the launch takes plain pointers (graph-capturable like the others).  One thread per output element,
 * consecutive threads on consecutive addresses of a destination.
 * CMPC_ERR_ARG: NULL dims, z or row; a NULL kkt / iters / status whose destination is set; batch < 0; N < 1;
 * nx < 1 or nx > CMPC_MAX_NX; nu < 1 or nu > CMPC_MAX_NU; ns < 0 or ns > CMPC_MAX_NS; look_col outside [0, nx).
 * batch == 0: CMPC_OK without a launch.  cmpc.scenarios.log_row is its numpy statement.
 * ---------------------------------------------------------------------- */
typedef struct { int batch, nx, nu, ns, N; int look_col; } cmpc_log_dims;   /* look_col: state column of the look-ahead */
typedef struct {            /* DEVICE pointers to ONE round's rows; any may be NULL (that part is skipped) */
    double *state;          /* batch x nx : z[b, 0 .. nx)                       = xPred[0]               */
    double *u;              /* batch x nu : z[b, (nx+ns)(N+1) .. +nu)           = uPred[0]               */
    double *look_ahead;     /* batch      : z[b, (nx+ns)N + look_col] - z[b, look_col]  (one subtraction) */
    double *kkt; int *iters, *status;     /* batch: copies of the round's solver outputs                 */
} cmpc_log_row;
int cmpc_round_log_dev(cmpc_ctx* ctx, const cmpc_log_dims* dims, const double* z /* batch x nz */, const double* kkt,
                       const int* iters, const int* status, const cmpc_log_row* row, void* hip_stream);

/* The log on the round handles: cmpc_lpv_rounds_step(h, 100, ...) / cmpc_di_rounds_step(h, 100, ...) leave every
 * round's states, inputs, look-ahead, solver outputs and solve time readable afterwards, with no host
 * synchronisation or copy per round.
 *
 * _log_enable (after create; the handle's structs and ABI are unchanged) allocates a device ring of `capacity`
 * rounds and 2 x capacity events, freed by _destroy.  Rounds are counted from create (both handles); the log
 * covers rounds from the handle's round count at the moment of the call, round r in row r mod capacity.  With
 * the log on, a round ends — after its exchange — with cmpc_round_log_dev on the round's z and its kkt / iters /
 * status (the DI handle: the history-ring row the solver wrote):
 *   LPV: nx, nu, ns = 9, 2, 3, look_col = 6 (s: the reference's plan_dist);
 *   DI:  nx = 2 dim, nu = dim, ns = 3, look_col = 0 (the predicted advance along the road).
 * A round that halts the LPV loop is logged (it ran); a round whose solver call returns an API error is not.
 * solve_ms: an event pair on the context's stream around the round's solver call (cmpc_solve_lpv_batch_dev /
 * cmpc_di_round_dev) and nothing else; nothing waits on the events during the step, _log_read resolves them
 * after its own synchronise.  It is the WHOLE BATCH's launch time — the same for every agent of the rank, not a
 * per-agent solve time (the reference times each agent's OSQP call).  Milliseconds.
 * CMPC_LOG_SEPARATION: after the exchange, cmpc_nbr_select_dev with nb = 1, window (0, 0), on the exchange
 * buffer, straight into the ring: `nearest` = each local agent's nearest other agent at stage 0 (global index)
 * and `sep2` the squared distance — cmpc.scenarios.select_neighbours(traj_all, 1, (0, 0), rows = the local
 * agents, return_dist2 = True) on the buffer as that round's exchange left it (stage 0 = every agent's logged
 * xPred[0] position).  Needs n_total >= 2, and not a sharded CMPC_ROUNDS_HOST_EXCHANGE handle (its exchange
 * happens after the step: the other ranks' rows would be stale).
 * With the log off every launch and every output of a step is what it was.
 *
 * _log_range: the rounds the ring holds now, [*first_round, *first_round + *count); (k, 0) before the first
 * logged round, k the handle's round count at enable.
 * _log_read: rounds [first_round, first_round + count) into HOST arrays with leading dimension count (any may be
 * NULL).  Synchronises the host.
 * CMPC_ERR_ARG: a NULL handle; _log_enable twice, capacity < 1, an unknown flag, CMPC_LOG_SEPARATION with
 * n_total < 2 or on a sharded host-exchange handle; _log_range / _log_read without _log_enable; a NULL output
 * struct; first_round < 0, count < 0; a round that has not run, ran before _log_enable, or has been overwritten
 * (count == 0 inside the rounds run so far: CMPC_OK); sep2 / nearest without CMPC_LOG_SEPARATION. */
#define CMPC_LOG_SEPARATION 1
typedef struct {            /* HOST pointers, any may be NULL; leading dimension = count */
    double *state, *u, *look_ahead, *kkt; int *iters, *status;   /* count x batch [x nx | x nu] */
    double *sep2; int *nearest;                                  /* count x batch (CMPC_LOG_SEPARATION) */
    double *solve_ms;                                            /* count: the batch's solver launch, ms */
} cmpc_rounds_log;
int cmpc_lpv_rounds_log_enable(cmpc_lpv_rounds* h, int capacity, int flags);
int cmpc_lpv_rounds_log_range(cmpc_lpv_rounds* h, int* first_round, int* count);
int cmpc_lpv_rounds_log_read(cmpc_lpv_rounds* h, int first_round, int count, const cmpc_rounds_log* host_out);
int cmpc_di_rounds_log_enable(cmpc_di_rounds* h, int capacity, int flags);
int cmpc_di_rounds_log_range(cmpc_di_rounds* h, int* first_round, int* count);
int cmpc_di_rounds_log_read(cmpc_di_rounds* h, int first_round, int count, const cmpc_rounds_log* host_out);

/* ------------------------------------------------------------------------
 * Consensus rounds for any linear agent model: the third family.  An agent is given by its own A_k, B_k
 * (cmpc_mpc_data, any structured linear time-varying model cmpc_solve_mpc_batch_dev takes), its own stage rows
 * C_own / h_own (mo per stage), its own linear cost qlin_own and the two state columns ix, iy that hold its
 * position.  Per round the builder appends the nb collision rows (compute_plane.py:41-68) and adds the coverage
 * term (misc.py:10-18) from the exchanged trajectories; the advance applies the round update of
 * LPV_HP_N_main.py:106-117.  DEVICE pointers, stream-ordered, no host synchronisation, no scratch,
 * graph-capturable.  The double-integrator family above is the special case ix, iy = 0, 1, mo = 4 with its four
 * constant rows and two constant cost entries in the caller's arrays (cmpc.scenarios.lin_of_di), bit for bit.
 *
 * cmpc_lin_build_dev: the rule.  Every expression is rounded as written (no fma: the bits of numpy;
 * cmpc.scenarios.lin_rows is its numpy statement).  For local agent b (global index g = self_offset + b), with
 * own = traj_all[g] (traj_all: n_total x (N+1) x 2) and mc = mo + nb:
 *   qlin[b,k,:] = qlin_own[b,k,:]                                            k = 0..N
 *   stage k = 1..N, written at row index k-1 of C (batch x N x mc x nx) and h (batch x N x mc):
 *     rows r < mo:   C[b,k-1,r,:] = C_own[b,k-1,r,:],  h[b,k-1,r] = h_own[b,k-1,r]
 *     row mo + i, neighbour i < nb, j = nbr[b,i]:
 *       e = own[k-1], n = traj_all[j,k-1];  dx = n_x - e_x, dy = n_y - e_y;  nrm = sqrt(dx*dx + dy*dy)
 *       ax = dx/nrm, ay = dy/nrm;  bb = -0.5*(ax*(e_x + n_x) + ay*(e_y + n_y))
 *       C[b,k-1,mo+i,:] = 0 except [ix] = ax, [iy] = ay;  h[b,k-1,mo+i] = -min_dist/2 - bb
 *     coverage, from row k:  qx = own[k]_x - traj_all[j,k]_x, qy likewise;
 *       wgt = (2*min_dist - sqrt(qx*qx + qy*qy))/nb;  px = px + wq*wgt*ax, py = py + wq*wgt*ay, accumulated
 *       from 0.0 in neighbour order;  then qlin[b,k,ix] += px, qlin[b,k,iy] += py
 *   stage 0 gets no coverage term.
 * A neighbour on the agent's own point (nrm = 0) gives NaN rows and a NaN cost at that stage, for that agent
 * only, as in both other families: keep j != g and distinct positions (cmpc_nbr_select_dev never returns g).
 * One workgroup per agent: the copies with consecutive lanes on consecutive addresses, the planes one lane per
 * stage.  nbr: batch x nb global indices (may be NULL when nb == 0), not range-checked on the device.
 *
 * cmpc_lin_advance_dev: from z (batch x nz, reference layout, nxe = nx + ns, nz = nxe(N+1) + 2 nu N):
 *   x0[b,:] <- z[b, nxe .. nxe+nx),  u_prev[b,:] <- z[b, nxe(N+1) .. +nu),
 *   traj_local[b,k,:] <- (z[b, k nxe + ix], z[b, k nxe + iy]),  k = 0..N.
 * An agent whose z holds any non-finite value is not advanced: its x0, u_prev and traj_local rows stay as they
 * were (cmpc_lpv_advance_dev's rule), so no NaN reaches a neighbour.
 *
 * cmpc_lin_round_dev: cmpc_lin_build_dev into data->qlin / C / h (written despite the const, as
 * cmpc_di_solve_dev), cmpc_solve_mpc_batch_dev(mpc_dims, w, data, out, opts), cmpc_lin_advance_dev(z = out->z,
 * x0 = data->x0, u_prev = data->u_prev: written despite the const).  Every solver flag means what it means on
 * cmpc_solve_mpc_batch_dev (rescue, polish, certify, the LPV flags, order, stamps; CMPC_FLAG_LPV_AUTO stays
 * CMPC_ERR_ARG); solver errors come back unchanged.  traj_all is only read (the Jacobi round); the exchange
 * traj_local -> traj_all is the caller's next step, and traj_local must not alias traj_all.
 *
 * CMPC_ERR_ARG: a NULL struct or required pointer (C_own / h_own may be NULL when mo == 0, nbr when nb == 0);
 * ix == iy, or either outside [0, nx); nb < 0, mo < 0 or mo + nb > CMPC_MAX_MC; nx outside 1..CMPC_MAX_NX;
 * N < 1, batch < 0 or self_offset < 0; the advance: ns outside 0..CMPC_MAX_NS, nu outside 1..CMPC_MAX_NU; the
 * round: mpc_dims not describing the same agents (nx, N, batch not equal, or mc != mo + nb).  batch == 0:
 * CMPC_OK without a launch.
 * ---------------------------------------------------------------------- */
typedef struct { int ix, iy; double min_dist, wq; } cmpc_lin_params;      /* position = state columns ix, iy */
typedef struct { int batch, N, nb, self_offset; int nx, mo; } cmpc_lin_dims; /* mo own rows per stage; mc = mo + nb */
typedef struct {            /* DEVICE pointers, per agent, batch-major, only read */
    const double* qlin_own; /* batch x (N+1) x nx */
    const double* C_own;    /* batch x N x mo x nx  (may be NULL when mo == 0) */
    const double* h_own;    /* batch x N x mo       (may be NULL when mo == 0) */
} cmpc_lin_own;

int cmpc_lin_build_dev(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_lin_dims* dims,
                       const int* nbr /* batch x nb, global agent indices */, const cmpc_lin_own* own,
                       const double* traj_all /* n_total x (N+1) x 2 */, double* qlin /* batch x (N+1) x nx */,
                       double* C /* batch x N x (mo+nb) x nx */, double* h /* batch x N x (mo+nb) */,
                       void* hip_stream);
int cmpc_lin_advance_dev(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_lin_dims* dims, int ns, int nu,
                         const double* z /* batch x nz */, double* x0 /* batch x nx */,
                         double* u_prev /* batch x nu */, double* traj_local /* batch x (N+1) x 2 */,
                         void* hip_stream);
int cmpc_lin_round_dev(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_lin_dims* ldims, const int* nbr,
                       const cmpc_lin_own* own, const double* traj_all, const cmpc_mpc_dims* mpc_dims,
                       const cmpc_mpc_weights* w, const cmpc_mpc_data* data, const cmpc_mpc_out* out,
                       const cmpc_opts* opts, double* traj_local /* batch x (N+1) x 2 */, void* hip_stream);

/* The round handle of the family, built as cmpc_di_rounds is (sharding, exchange, history ring, log: see
 * there).  A round, on the context's stream:
 *   1. CMPC_ROUNDS_RESELECT and nb > 0: cmpc_nbr_select_dev, window (0, 0), into the handle's table;
 *   2. cmpc_lin_round_dev on the handle's buffers; with CMPC_ROUNDS_LPT, from the second round on,
 *      cmpc_opts.order = the handle's order buffer;
 *   3. CMPC_ROUNDS_LPT: cmpc_order_by_iters_dev of this round's iteration counts into the order buffer;
 *   4. the exchange (a device copy, the context's communicator, or the host's: CMPC_ROUNDS_HOST_EXCHANGE);
 *   5. with the log on, the log row: nx, nu, ns of the handle's dims, look_col = ix.
 * No halt rule (CMPC_ROUNDS_NO_HALT is accepted and has no effect).  A, B, qlin_own, C_own, h_own are uploaded
 * once and never changed by the handle (CMPC_FLAG_LTI is set when A and B pass cmpc_di_rounds_create's test).
 * opts->flags go to the solver unchanged; opts->stamps and opts->order are ignored.  _set_state replaces the
 * predicted state of the next round by a measured one (HOST pointers, batch x nx / batch x nu; either may be
 * NULL: that part stays).  _read, _history, _get_traj, _set_traj, _destroy and the log functions are
 * cmpc_di_rounds_*'s.
 * CMPC_ERR_ARG at create: what cmpc_di_rounds_create lists (its `dim` and `4 + nb` rules replaced by the
 * dimension rules of cmpc_lin_build_dev / _advance_dev above; init->C_own / h_own may be NULL when mo == 0).
 * CMPC_ROUNDS_RESELECT keeps cmpc_nbr_select_dev's nb <= CMPC_MAX_MC - 4. */
typedef struct cmpc_lin_rounds cmpc_lin_rounds;
typedef struct { int n_total, batch, self_offset, N, nb, flags, history; int nx, nu, ns, mo; } cmpc_lin_rounds_dims;
typedef struct {    /* HOST pointers, this rank's agents, copied at create */
    const double *A, *B;        /* batch x N x nx x nx, batch x N x nx x nu */
    const double *x0, *u_prev;  /* batch x nx, batch x nu */
    const double *qlin_own, *C_own, *h_own;   /* as cmpc_lin_own */
    const int* nbr;             /* batch x nb global indices (checked: 0 <= j < n_total) */
    const double* traj;         /* n_total x (N+1) x 2 initial exchange buffer (required) */
} cmpc_lin_rounds_init;
typedef struct {    /* HOST pointers, any may be NULL: the latest round of this rank's agents */
    double *z, *kkt;            /* batch x nz (nz = (nx + ns)(N+1) + 2 nu N), batch */
    int *iters, *status;        /* batch */
    double *x0, *u_prev;        /* batch x nx, batch x nu: the next round's initial state and previous input */
    int* nbr;                   /* batch x nb: the table the latest round used */
} cmpc_lin_rounds_out;

/* w: ns slacks and mc = mo + nb rows, copied at create. */
int cmpc_lin_rounds_create(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_mpc_weights* w,
                           const cmpc_lin_rounds_dims* dims, const cmpc_lin_rounds_init* init, const cmpc_opts* opts,
                           cmpc_lin_rounds** out);
int cmpc_lin_rounds_step(cmpc_lin_rounds* h, int rounds, int* rounds_done);
int cmpc_lin_rounds_read(cmpc_lin_rounds* h, const cmpc_lin_rounds_out* host_out);
int cmpc_lin_rounds_history(cmpc_lin_rounds* h, int first_round, int count, double* kkt, int* iters, int* status);
int cmpc_lin_rounds_get_traj(cmpc_lin_rounds* h, double* traj_local);
int cmpc_lin_rounds_set_traj(cmpc_lin_rounds* h, const double* traj_all);
int cmpc_lin_rounds_set_state(cmpc_lin_rounds* h, const double* x0, const double* u_prev);
int cmpc_lin_rounds_destroy(cmpc_lin_rounds* h);
int cmpc_lin_rounds_log_enable(cmpc_lin_rounds* h, int capacity, int flags);
int cmpc_lin_rounds_log_range(cmpc_lin_rounds* h, int* first_round, int* count);
int cmpc_lin_rounds_log_read(cmpc_lin_rounds* h, int first_round, int count, const cmpc_rounds_log* host_out);

/* ------------------------------------------------------------------------
 * Time-varying agents of the family: a stage table that slides one stage per round.  A round is a control step,
 * so round r of an agent whose model, reference or bounds change along its future plans with A_r .. A_{r+N-1} and
 * the own data of stages r .. r+N.  The future is given as a table of stages (a successive-linearisation table, a
 * periodic model, a reference-speed profile, a bound that tightens along a road).
 *
 * A STAGE TABLE holds, per agent, T >= 1 rows indexed by absolute stage tau:
 *   A    batch x T x nx x nx     x_{tau+1} = A_tau x_tau + B_tau u_tau
 *   B    batch x T x nx x nu
 *   qlin batch x T x nx          own linear cost on x_tau
 *   C    batch x T x mo x nx     own rows on x_tau      (NULL when mo == 0)
 *   h    batch x T x mo
 * row(tau) = tau mod T with CMPC_TABLE_PERIODIC, min(tau, T-1) with CMPC_TABLE_HOLD (past its end the table holds
 * its last stage).  The window at time t >= 0 is
 *   A_win[b,k]    = A[b,row(t+k)]                      k = 0..N-1   (B likewise)
 *   qlin_own[b,k] = qlin[b,row(t+k)]                   k = 0..N
 *   C_own[b,k-1]  = C[b,row(t+k)],  h_own likewise     k = 1..N
 * every value copied bit for bit (-0.0 stays -0.0, a NaN stays a NaN); N + 1 > T is allowed (HOLD repeats the last
 * row, PERIODIC wraps as often as needed).  cmpc.scenarios.lin_table_rows / lin_window are the numpy statement.
 *
 * cmpc_lin_table_build_dev: a round's whole build in one launch.  A_win, B_win are written into A (batch x N x nx
 * x nx) and B (batch x N x nx x nu), and qlin, C, h are exactly cmpc_lin_build_dev's rule applied to that window,
 * the own data read through row() straight from the table (no intermediate window, no second launch).  One
 * workgroup per agent, no LDS, no scratch, stream-ordered, graph-capturable; t is a launch argument.
 *
 * cmpc_lin_table_round_dev: cmpc_lin_round_dev with that build: cmpc_lin_table_build_dev into data->A / B / qlin /
 * C / h (written despite the const), cmpc_solve_mpc_batch_dev, cmpc_lin_advance_dev into data->x0 / u_prev and
 * traj_local.  Every argument rule, the solver's included, is checked before the first launch; solver flags
 * mean what they mean on cmpc_solve_mpc_batch_dev (CMPC_FLAG_LTI is the caller's promise about the WINDOW).
 *
 * CMPC_ERR_ARG: what cmpc_lin_build_dev / cmpc_lin_round_dev list; T < 1; a mode other than 0 or 1; t < 0 or
 * t > INT_MAX - N; nu outside 1..CMPC_MAX_NU (the round: mpc_dims->nu is the table's); a NULL table array (C / h
 * may be NULL when mo == 0); a NULL output.  batch == 0: CMPC_OK without a launch.
 * ---------------------------------------------------------------------- */
#define CMPC_TABLE_HOLD 0
#define CMPC_TABLE_PERIODIC 1
typedef struct { int T, mode; } cmpc_lin_table_dims;
typedef struct { const double *A, *B, *qlin, *C, *h; } cmpc_lin_table;   /* DEVICE pointers, only read */

int cmpc_lin_table_build_dev(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_lin_dims* dims, int nu,
                             const cmpc_lin_table_dims* tdims, const cmpc_lin_table* table, int t, const int* nbr,
                             const double* traj_all, double* A, double* B, double* qlin, double* C, double* h,
                             void* hip_stream);
int cmpc_lin_table_round_dev(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_lin_dims* ldims, const int* nbr,
                             const cmpc_lin_table_dims* tdims, const cmpc_lin_table* table, int t,
                             const double* traj_all, const cmpc_mpc_dims* mpc_dims, const cmpc_mpc_weights* w,
                             const cmpc_mpc_data* data, const cmpc_mpc_out* out, const cmpc_opts* opts,
                             double* traj_local /* batch x (N+1) x 2 */, void* hip_stream);

/* The round handle over a stage table: cmpc_lin_rounds_create_table returns the handle type of
 * cmpc_lin_rounds_create, so _step, _read, _history, _get_traj / _set_traj, _set_state, _destroy and the log
 * functions work on it unchanged.  The handle keeps the table on the device and a time t (t0 at create); step 2 of
 * a round is cmpc_lin_table_round_dev at t.  After a round that ran, t <- (t + 1) mod T (PERIODIC) or
 * min(t + 1, T - 1) (HOLD: from there every window row already reads the last stage); a round whose solver call
 * returns an API error does not advance t.  CMPC_FLAG_LTI is set only when every row of the whole A and B tables
 * is bit-equal to row 0 (and finite); a _table_write that carries A or B clears it.
 *   _get_time / _set_time: the time of the next round; _set_time takes 0 <= t < T.
 *   _table_write: HOST arrays batch x count x ... (the table's shapes with count for T) into rows [first_row,
 *     first_row + count) of every agent; no wrap (the caller splits a wrapped write); any array may be NULL: that
 *     part stays as it was.  Synchronises.  A PERIODIC table whose consumed rows the host overwrites is a ring
 *     for online re-linearisation.
 * On a handle of cmpc_lin_rounds_create _get_time gives 0; _set_time and _table_write return CMPC_ERR_ARG.
 * CMPC_ERR_ARG at create: what cmpc_lin_rounds_create lists (the table arrays for its A, B, qlin_own, C_own,
 * h_own); T < 1; a mode other than 0 or 1; t0 < 0 or t0 >= T.  _table_write: first_row < 0, count < 0,
 * first_row + count > T, a NULL struct. */
typedef struct {    /* HOST pointers, this rank's agents, copied at create */
    int T, mode, t0;
    const double *A, *B, *qlin, *C, *h;   /* the table, shapes as above (C / h may be NULL when mo == 0) */
    const double *x0, *u_prev;            /* as cmpc_lin_rounds_init */
    const int* nbr;
    const double* traj;
} cmpc_lin_rounds_table_init;

int cmpc_lin_rounds_create_table(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_mpc_weights* w,
                                 const cmpc_lin_rounds_dims* dims, const cmpc_lin_rounds_table_init* init,
                                 const cmpc_opts* opts, cmpc_lin_rounds** out);
int cmpc_lin_rounds_get_time(cmpc_lin_rounds* h, int* t);
int cmpc_lin_rounds_set_time(cmpc_lin_rounds* h, int t);
int cmpc_lin_rounds_table_write(cmpc_lin_rounds* h, int first_row, int count, const cmpc_lin_table* host_rows);

/* ------------------------------------------------------------------------
 * Consensus steps of the family: a control step that repeats build, solve, publish and exchange at a fixed state
 * and a fixed table time until the published positions agree, and only then advances (the inner loop of
 * NL_EU_N_main.py:105-162 on the Jacobi round above).  A plain round cuts every agent's collision planes against
 * plans its neighbours have already abandoned; an inner round cuts them against the plans of the round before.
 *
 * cmpc_lin_publish_dev: one inner round's publication and its convergence test, in one launch (one wavefront per
 * agent, no LDS, no scratch, stream-ordered, graph-capturable).  Every expression is rounded as written
 * (cmpc.scenarios.lin_publish is its numpy statement).  For local agent b, with g = self_offset + b,
 * prev = traj_all[g] (traj_all: n_total x (N+1) x 2), nxe = nx + ns and
 *   new[k] = (z[b, k nxe + ix], z[b, k nxe + iy]),  k = 0..N:
 *   z[b] holds a non-finite value anywhere in its nz entries:
 *     traj_local[b] <- prev, bit for bit;  close[b] = 0;  delta[b] = NaN.
 *     (Not cmpc_lin_advance_dev's "stays as it was": after the exchange the agent's row of traj_all is unchanged
 *     whatever traj_local held before.)
 *   z[b] finite:
 *     traj_local[b] <- new (copies: -0.0 stays -0.0);
 *     close[b] = 1 exactly when |prev_e - new_e| <= atol + rtol * |new_e| for all 2(N+1) entries e — the test of
 *       cmpc_ocd_converged_dev with x_old = prev, x_pred = new: a NaN prev_e is never close, and an infinite one
 *       is not close under any finite atol;
 *     delta[b] = max over e of |prev_e - new_e|, NaN when any term is NaN (numpy's max, not fmax).
 *   *not_close += the number of agents with close == 0: one vector atomic add from one lane of each such agent, so
 *   the caller zeroes *not_close on the stream first (the handle below does).
 * close, delta and not_close may each be NULL: that output is skipped, the others are unchanged.  traj_local must
 * not alias traj_all.
 * CMPC_ERR_ARG: what cmpc_lin_advance_dev lists; a NULL traj_all; atol or rtol negative or NaN (+inf is allowed).
 * batch == 0: CMPC_OK without a launch.
 *
 * The stopping rule (cmpc.scenarios.consensus_stop is its statement).  Inner rounds are numbered j = 1, 2, ...;
 * round 1 compares against the previous step's plan and is not used (its count is recorded).  For j >= 2, streak
 * = the number of consecutive rounds, ending at j, whose node-wide not_close was 0; agreed becomes true the first
 * time streak >= need and stays true; the step stops after round j when j >= max_rounds, or when agreed and
 * j >= min_rounds.  This is the reference's loop (cmpc.ocd.OCDLoopState) with min_rounds = min_it_OCD + 1, need =
 * it_conv + 1, max_rounds = max_it_OCD + 2; a NULL cmpc_consensus_opts gives the reference's 3, 2, 12, atol 0.01,
 * rtol 1e-5.
 *
 * cmpc_lin_rounds_step_consensus runs `steps` consensus steps on a handle of cmpc_lin_rounds_create or
 * _create_table.  One step, on the context's stream:
 *   1. CMPC_ROUNDS_RESELECT: cmpc_nbr_select_dev, once; the log's first event;
 *   2. per inner round: cmpc_lin_build_dev (cmpc_lin_table_build_dev at the handle's time t);
 *      cmpc_solve_mpc_batch_dev into this step's history row; with CMPC_ROUNDS_LPT cmpc_order_by_iters_dev (the
 *      order is used from the second solve of the handle on; results do not depend on it); *not_close <- 0;
 *      cmpc_lin_publish_dev; the exchange; sharded over the communicator, cmpc_comm_sum_i32 of the count; a 4-byte
 *      read-back and one stream wait (as cmpc_lpv_rounds_step for its halt rule);
 *   3. the log's second event; cmpc_lin_advance_dev from the final z (it rewrites traj_local with the values
 *      already exchanged: no second exchange); the log row; the round count and t move on once.
 * A consensus step is ONE round for _history, the log and t; its history row holds the last inner round's kkt,
 * iters and status.  Plain and consensus steps may be mixed on one handle.  With max_rounds == 1 a step leaves
 * every array a plain cmpc_lin_rounds_step(h, 1) leaves, byte for byte.  A solver error is returned unchanged and
 * the step is not counted: x0, u_prev and t are untouched; traj_all may hold the inner rounds already exchanged.
 * steps_done / inner_total (may be NULL): the steps completed and the inner rounds they ran.
 * CMPC_ERR_ARG (nothing is written): a NULL handle; steps < 0; min_rounds < 1, need < 1 or max_rounds <
 * min_rounds; atol or rtol negative or NaN; a sharded handle with CMPC_ROUNDS_HOST_EXCHANGE (the exchange lies
 * inside the step).
 *
 * cmpc_lin_rounds_consensus_read (HOST pointers, any may be NULL), for the latest consensus step: its inner round
 * count; agreed (0 / 1); not_close[j-1] = the node-wide count after inner round j, for j <= min(cap,
 * inner_rounds) (entry 0: against the previous step's plan); this rank's close and delta (batch each) of the last
 * inner round.  Before the first consensus step: 0 rounds, not agreed, zeros.  CMPC_ERR_ARG: a NULL handle or
 * struct, cap < 0.
 * ---------------------------------------------------------------------- */
int cmpc_lin_publish_dev(cmpc_ctx* ctx, const cmpc_lin_params* prm, const cmpc_lin_dims* dims, int ns, int nu,
                         const double* z /* batch x nz */, const double* traj_all /* n_total x (N+1) x 2 */,
                         double atol, double rtol, double* traj_local /* batch x (N+1) x 2 */,
                         int* close /* batch, may be NULL */, double* delta /* batch, may be NULL */,
                         int* not_close /* device int, may be NULL */, void* hip_stream);

typedef struct { int min_rounds, need, max_rounds; double atol, rtol; } cmpc_consensus_opts;   /* NULL: the defaults */
typedef struct {    /* HOST pointers, any may be NULL */
    int *inner_rounds, *agreed;
    int* not_close;             /* cap entries */
    int cap;
    int* close;                 /* batch */
    double* delta;              /* batch */
} cmpc_consensus_out;
int cmpc_lin_rounds_step_consensus(cmpc_lin_rounds* h, int steps, const cmpc_consensus_opts* co, int* steps_done,
                                   int* inner_total);
int cmpc_lin_rounds_consensus_read(cmpc_lin_rounds* h, const cmpc_consensus_out* host_out);

/* ------------------------------------------------------------------------
 * Positions in three dimensions on the linear-model family (cmpc_lin3_*, cmpc_nbr_select3_dev): the coupling of
 * agents that move in space (the 3-D double integrator: nx = 6, nu = 3).  The position is three state columns ix,
 * iy, iz, pairwise different and each in [0, nx), and every exchange buffer is x 3: traj_all n_total x (N+1) x 3,
 * traj_local batch x (N+1) x 3.  Everything that does not touch a position is the planar family's, and each entry
 * point below has the signature, the launch shape (one wavefront per agent, no LDS, no scratch, stream-ordered,
 * graph-capturable) and the error rules of its namesake without the 3, with cmpc_lin3_params for cmpc_lin_params.
 * Every expression is rounded as written (no fma) and sums run left to right; cmpc.scenarios.lin_rows /
 * lin_advance / lin_publish / select_neighbours with `iz` in prm (a 3-column buffer) are the numpy statements.
 *
 * cmpc_lin3_build_dev, cmpc_lin3_table_build_dev: cmpc_lin_build_dev's rule with, for neighbour i of stage k,
 * e = own[k-1], n = traj_all[j,k-1]:
 *       dx, dy, dz = n - e;  nrm = sqrt(dx*dx + dy*dy + dz*dz);  ax, ay, az = dx/nrm, dy/nrm, dz/nrm
 *       bb = -0.5*(ax*(e_x + n_x) + ay*(e_y + n_y) + az*(e_z + n_z))
 *       C[b,k-1,mo+i,:] = 0 except [ix] = ax, [iy] = ay, [iz] = az;  h[b,k-1,mo+i] = -min_dist/2 - bb
 *     coverage, from row k:  qx, qy, qz = own[k] - traj_all[j,k];
 *       wgt = (2*min_dist - sqrt(qx*qx + qy*qy + qz*qz))/nb;  px = px + wq*wgt*ax, py, pz likewise, accumulated
 *       from 0.0 in neighbour order;  then qlin[b,k,ix] += px, qlin[b,k,iy] += py, qlin[b,k,iz] += pz
 *   stage 0 gets no coverage term; the own rows and the own cost are copied as in the planar rule.  A neighbour on
 *   the agent's own 3-D point gives NaN for that agent and that stage only: two agents over one ground point at
 *   different altitudes have finite rows.  When every position has the same third coordinate, dz = 0 and the rows
 *   and the cost are the planar builder's, with a zero in column iz.
 * cmpc_lin3_advance_dev, cmpc_lin3_publish_dev: new[k] = (z[k nxe + ix], z[k nxe + iy], z[k nxe + iz]), 3(N+1)
 *   entries per agent; the non-finite guard, the allclose test, delta with numpy's max, the atomic count and the
 *   copy (-0.0 stays -0.0) are cmpc_lin_advance_dev's / cmpc_lin_publish_dev's.
 * cmpc_lin3_round_dev, cmpc_lin3_table_round_dev: the planar rounds with those builds and that advance.
 * cmpc_nbr_select3_dev: cmpc_nbr_select_dev with score(g, j) = min over k in [k0, k1] of (dx*dx + dy*dy + dz*dz);
 *   the NaN, tie-break, self-exclusion and error rules are unchanged.
 *
 * cmpc_lin_rounds_create3 / cmpc_lin_rounds_create_table3 are cmpc_lin_rounds_create / _create_table with
 * cmpc_lin3_params and an x 3 initial buffer (init->traj: n_total x (N+1) x 3).  They return the same
 * cmpc_lin_rounds, and every other handle function works on it unchanged: _step, _step_consensus,
 * _consensus_read, _read, _history, _set_state, _get_time, _set_time, _table_write, the log functions, _destroy.
 * On such a handle _get_traj / _set_traj move 3(N+1) doubles per agent, CMPC_ROUNDS_RESELECT and
 * CMPC_LOG_SEPARATION run cmpc_nbr_select3_dev (sep2 is the squared 3-D distance), the log's look_col stays ix,
 * and the exchange (device copy, communicator, host) moves the longer rows.  cmpc_lin_rounds_pos_dim gives 2 or 3.
 *
 * CMPC_ERR_ARG: what the planar namesake lists; iz equal to ix or iy; iz outside [0, nx).
 * ---------------------------------------------------------------------- */
typedef struct { int ix, iy, iz; double min_dist, wq; } cmpc_lin3_params; /* position = state columns ix, iy, iz */

int cmpc_lin3_build_dev(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_lin_dims* dims,
                        const int* nbr /* batch x nb, global agent indices */, const cmpc_lin_own* own,
                        const double* traj_all /* n_total x (N+1) x 3 */, double* qlin /* batch x (N+1) x nx */,
                        double* C /* batch x N x (mo+nb) x nx */, double* h /* batch x N x (mo+nb) */,
                        void* hip_stream);
int cmpc_lin3_advance_dev(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_lin_dims* dims, int ns, int nu,
                          const double* z /* batch x nz */, double* x0 /* batch x nx */,
                          double* u_prev /* batch x nu */, double* traj_local /* batch x (N+1) x 3 */,
                          void* hip_stream);
int cmpc_lin3_publish_dev(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_lin_dims* dims, int ns, int nu,
                          const double* z /* batch x nz */, const double* traj_all /* n_total x (N+1) x 3 */,
                          double atol, double rtol, double* traj_local /* batch x (N+1) x 3 */,
                          int* close /* batch, may be NULL */, double* delta /* batch, may be NULL */,
                          int* not_close /* device int, may be NULL */, void* hip_stream);
int cmpc_lin3_round_dev(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_lin_dims* ldims, const int* nbr,
                        const cmpc_lin_own* own, const double* traj_all, const cmpc_mpc_dims* mpc_dims,
                        const cmpc_mpc_weights* w, const cmpc_mpc_data* data, const cmpc_mpc_out* out,
                        const cmpc_opts* opts, double* traj_local /* batch x (N+1) x 3 */, void* hip_stream);
int cmpc_lin3_table_build_dev(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_lin_dims* dims, int nu,
                              const cmpc_lin_table_dims* tdims, const cmpc_lin_table* table, int t, const int* nbr,
                              const double* traj_all /* n_total x (N+1) x 3 */, double* A, double* B, double* qlin,
                              double* C, double* h, void* hip_stream);
int cmpc_lin3_table_round_dev(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_lin_dims* ldims, const int* nbr,
                              const cmpc_lin_table_dims* tdims, const cmpc_lin_table* table, int t,
                              const double* traj_all, const cmpc_mpc_dims* mpc_dims, const cmpc_mpc_weights* w,
                              const cmpc_mpc_data* data, const cmpc_mpc_out* out, const cmpc_opts* opts,
                              double* traj_local /* batch x (N+1) x 3 */, void* hip_stream);
int cmpc_nbr_select3_dev(cmpc_ctx* ctx, const cmpc_nbr_dims* dims, const double* traj_all /* n_total x (N+1) x 3 */,
                         int* nbr /* batch x nb */, double* dist2 /* batch x nb, may be NULL */, void* hip_stream);
int cmpc_lin_rounds_create3(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_mpc_weights* w,
                            const cmpc_lin_rounds_dims* dims, const cmpc_lin_rounds_init* init, const cmpc_opts* opts,
                            cmpc_lin_rounds** out);
int cmpc_lin_rounds_create_table3(cmpc_ctx* ctx, const cmpc_lin3_params* prm, const cmpc_mpc_weights* w,
                                  const cmpc_lin_rounds_dims* dims, const cmpc_lin_rounds_table_init* init,
                                  const cmpc_opts* opts, cmpc_lin_rounds** out);
int cmpc_lin_rounds_pos_dim(cmpc_lin_rounds* h, int* pos_dim /* 2, or 3 on a handle of the create3 forms */);

/* ------------------------------------------------------------------------
 * Consensus steps of the reference's LPV agents (cmpc_lpv_rounds_*): the same step on the handle that drives the
 * reference's own model.  The model is fixed within a step: every inner round linearises about the previous STEP's
 * prediction (the handle's x_last, u_last, u_old, last_rows, at its x0), exactly as a plain round does, and only the
 * coupling is iterated: the collision planes and the coverage weights are re-cut against the positions the round
 * before published.  Re-linearising about each inner round's own prediction does not settle on this model (a
 * single agent without neighbours keeps moving by 0.02 to 0.06 per round); DESIGN.md section 4 has the finding.
 *
 * cmpc_lpv_publish_dev: one inner round's publication, its convergence test and its feasibility count, in one launch
 * (one wavefront per agent, no LDS, no scratch, stream-ordered, graph-capturable).  dims = {batch, N, nb (not
 * read), self_offset} of cmpc_di_dims; z is batch x nz, nz = 12(N+1) + 4N.  For local agent b, with prev =
 * traj_all[self_offset + b] and new[k] = (z[b, 12k + 7], z[b, 12k + 8]), k = 0..N:
 *   traj_local[b], close[b], delta[b]: the rule of cmpc_lin_publish_dev above, every expression rounded as written
 *     (a non-finite value anywhere in z[b]: prev again bit for bit, close 0, delta NaN; otherwise new is copied,
 *     close = 1 exactly when |prev_e - new_e| <= atol + rtol |new_e| for all 2(N+1) entries, delta = the largest
 *     |prev_e - new_e|, NaN when any term is) — byte for byte what cmpc_lin_publish_dev gives with ix = 7, iy = 8,
 *     nx = 9, ns = 3, nu = 2 (the two kernels run one device function);
 *   counts[0] += the number of agents with close == 0;
 *   counts[1] += the number of agents whose status is not in {1, 2, -2}: the reference's feasibility rule, the one
 *     cmpc_lpv_advance_dev applies; skipped (counts[1] untouched) when status is NULL.
 * Each count is one vector atomic add from one lane of each counted agent: the caller zeroes counts (DEVICE int[2])
 * on the stream first.  close, delta and counts may each be NULL: that output is skipped, the others are unchanged.
 * traj_local must not alias traj_all.  cmpc.scenarios.lpv_publish is the numpy statement.
 * CMPC_ERR_ARG: a NULL dims, z, traj_all or traj_local; N < 1; batch < 0; self_offset < 0; atol or rtol negative or
 * NaN (+inf is allowed).  batch == 0: CMPC_OK without a launch.
 *
 * cmpc_lpv_rounds_step_consensus runs up to `steps` consensus steps; cmpc_consensus_opts, the stopping rule and the
 * NULL defaults are the linear family's above.  One step, on the context's stream:
 *   1. CMPC_ROUNDS_RESELECT: cmpc_nbr_select_dev, once; the log's first event;
 *   2. per inner round: cmpc_lpv_gather_dev; cmpc_solve_lpv_batch_dev on the handle's x0, x_last, u_last, u_old and
 *      last_rows, all untouched by inner rounds; counts <- 0 (8 bytes); cmpc_lpv_publish_dev; the exchange; sharded
 *      over the communicator, one cmpc_comm_sum_i32 of both counts; an 8-byte read-back and one stream wait; the
 *      node-wide not-close count joins the trace and the stopping rule is applied.  Without CMPC_ROUNDS_NO_HALT a
 *      node-wide infeasible count > 0 ends the inner loop after this round, whatever the stopping rule says;
 *   3. the log's second event; on the first step x_last goes from N+1 to N dense rows, as in cmpc_lpv_rounds_step;
 *      cmpc_lpv_advance_dev from the final z with status and infeasible NULL (the publish has counted; it rewrites
 *      traj_local with the values already exchanged: no second exchange); last_rows = N; the log row; the round
 *      count moves on once.
 * After a step the halt rule ended no further step of the call runs (steps_done < steps), as cmpc_lpv_rounds_step
 * after a round with an infeasible agent.  *infeasible (may be NULL): the node-wide count of the last inner round
 * run; steps_done / inner_total (may be NULL) as for the linear handle.  A consensus step is ONE round for the log
 * and the round count; its row holds the last inner round's outputs.  Plain and consensus steps may be mixed on one
 * handle.  With max_rounds == 1 a step leaves every array a plain cmpc_lpv_rounds_step(h, 1, ..) leaves, byte for
 * byte, x_last / u_last / u_old included.  A solver error is returned unchanged and the step is not counted: the
 * log row is abandoned, x0, x_last, u_last, u_old and last_rows are untouched; traj_all may hold the inner rounds
 * already exchanged.
 * CMPC_ERR_ARG (nothing is written): a NULL handle; steps < 0; min_rounds < 1, need < 1 or max_rounds <
 * min_rounds; atol or rtol negative or NaN; a sharded handle with CMPC_ROUNDS_HOST_EXCHANGE.
 * cmpc_lpv_rounds_consensus_read: as cmpc_lin_rounds_consensus_read.
 * ---------------------------------------------------------------------- */
int cmpc_lpv_publish_dev(cmpc_ctx* ctx, const cmpc_di_dims* dims /* batch, N, nb (not read), self_offset */,
                         const double* z /* batch x nz */, const double* traj_all /* n_total x (N+1) x 2 */,
                         const int* status /* batch, may be NULL */, double atol, double rtol,
                         double* traj_local /* batch x (N+1) x 2 */, int* close /* batch, may be NULL */,
                         double* delta /* batch, may be NULL */, int* counts /* DEVICE int[2], may be NULL */,
                         void* hip_stream);
int cmpc_lpv_rounds_step_consensus(cmpc_lpv_rounds* h, int steps, const cmpc_consensus_opts* co, int* steps_done,
                                   int* inner_total, int* infeasible);
int cmpc_lpv_rounds_consensus_read(cmpc_lpv_rounds* h, const cmpc_consensus_out* host_out);


/* ------------------------------------------------------------------------
 * Dense standard-form QP batch with MATLAB quadprog semantics (the MEX drop-in
 * for quadprog(H,f,A,b,Aeq,beq,lb,ub) as YALMIP calls it, callquadprog.m:63-69,
 * and the generic back end of the osqp_solve_qp adapter, LPV_Planner.py:192-249):
 *
 *   min 1/2 x'Hx + f'x   s.t.  A x <= b,  Aeq x = beq,  lb <= x <= ub
 *
 * HOST pointers, batch-major (problem p's block contiguous).  H n x n (its symmetric
 * part is used), A m_ineq x n, Aeq m_eq x n, row-major unless col_major (MATLAB
 * layout).  A/b, Aeq/beq, lb, ub may be NULL (absent); b_r, ub_i = +inf and
 * lb_i = -inf are inactive (their multipliers are exactly 0); b_r, ub_i = -inf,
 * lb_i = +inf or a NaN bound make the problem infeasible; all-zero constraint rows
 * are dropped (or make the problem infeasible).  A fixed variable lb_i == ub_i keeps
 * both bound rows active: both of its bound multipliers come back positive, and
 * only lambda_upper - lambda_lower, its equality multiplier, is determined.
 * exitflag: CMPC_QP_CONVERGED 1, CMPC_QP_MAXITER 0, CMPC_QP_INFEASIBLE -2,
 * CMPC_QP_UNBOUNDED -3, CMPC_QP_NONCONVEX -6 (quadprog's codes).  A solve that
 * ends short of opts->tol returns its best iterate (x and the multipliers of that
 * same iterate, residual its merit): 1 when that merit is below 1e3 tol; 0 when
 * opts->max_iter cut it off while the merit was still improving (a new best within
 * the last 3 iterations, so always for max_iter <= 3); otherwise -2 when the
 * primal residual, else -3 when the dual residual, is what stayed above 1e3 tol.
 * ---------------------------------------------------------------------- */
#define CMPC_QP_CONVERGED 1
#define CMPC_QP_MAXITER 0
#define CMPC_QP_INFEASIBLE (-2)
#define CMPC_QP_UNBOUNDED (-3)
#define CMPC_QP_NONCONVEX (-6)

typedef struct {
    int n, m_ineq, m_eq, batch;
    int col_major;
} cmpc_qp_dims;

typedef struct {
    const double *H, *f, *A, *b, *Aeq, *beq, *lb, *ub;
} cmpc_qp_data;

typedef struct {
    double* x;               /* batch x n */
    double* fval;            /* batch (may be NULL) */
    int* exitflag;           /* batch (may be NULL) */
    int* iters;              /* batch (may be NULL) */
    double* lambda_ineqlin;  /* batch x m_ineq (may be NULL) */
    double* lambda_eqlin;    /* batch x m_eq (may be NULL) */
    double* lambda_lower;    /* batch x n (may be NULL) */
    double* lambda_upper;    /* batch x n (may be NULL) */
    double* residual;        /* batch: final scaled KKT merit (may be NULL) */
} cmpc_qp_out;

int cmpc_solve_qp_batch(cmpc_ctx* ctx, const cmpc_qp_dims* dims, const cmpc_qp_data* host_in,
                        const cmpc_qp_out* host_out, const cmpc_opts* opts);

/* ------------------------------------------------------------------------
 * OCD coupling-dual round (planner/scripts/NL_EU_N_main.py:119-162; ROS variant
 * ROS/src/planner_experiments/src/OCD_ROS_main.py:200-239), DEVICE pointers:
 *   lam[b, s, k-1] += alpha * (dth - ||p_g(k) - p_j(k)||),  g = self_offset + b,
 *   j = nbr[b, s], for k = 1..N and only when g < j (the reference fills i < j);
 *   p from traj_all (n_total x (N+1) x 2).  alpha = 0.25 in the reference
 *   (config/NL/config.py:5-8), dth its safety distance.
 * cmpc_ocd_converged_dev: close[b] = numpy allclose(x_old[b], x_pred[b], atol, rtol)
 *   over `per` values per agent (the reference's convergence test, :143-162).
 * ---------------------------------------------------------------------- */
typedef struct {
    int batch, N, nb, self_offset;
} cmpc_ocd_dims;

int cmpc_ocd_update_dev(cmpc_ctx* ctx, const cmpc_ocd_dims* dims, double alpha, double dth, const int* nbr,
                        const double* traj_all, double* lam, void* hip_stream);
int cmpc_ocd_converged_dev(cmpc_ctx* ctx, int batch, int per, double atol, double rtol, const double* x_old,
                           const double* x_pred, int* close, void* hip_stream);

/* ----------------------------------------------------------------------
 * Multi-GPU exchange (RCCL over xGMI).  One process per GPU, one
 * context per process.  Replaces the per-round exchange of predicted trajectories —
 * the ROS topics of ROS/src/planner_experiments/src/LPV_ROS_main.py:66-77 (publish)
 * and :124-150 (subscribe), the in-process np.swapaxes of LPV_HP_N_main.py:117 —
 * for hosts that shard agents without torch (a MATLAB / C host).
 *
 *   cmpc_comm_id:   rank 0 creates the communicator id; the host hands its
 *                   CMPC_COMM_ID_BYTES bytes to every rank (MPI, a file, a socket).
 *   cmpc_comm_init: every rank joins (collective; blocks until all ranks joined).
 *   cmpc_allgather_trajectories: traj_all (nranks*count doubles, DEVICE) receives every
 *                   rank's traj_local (count doubles, DEVICE) in rank order; stream-ordered
 *                   (hip_stream as void*, 0 = default).  For the position exchange of a
 *                   round, count = local agents * (N+1) * 2.
 *   cmpc_comm_sum_i32: buf (count int32, DEVICE) <- its sum over every rank of the
 *                   communicator, in place, stream-ordered (one RCCL all-reduce).  The
 *                   rounds use it for the halt decision: the reference's loop stops for
 *                   every agent at once when one is infeasible (LPV_HP_N_main.py:102-111),
 *                   so every rank must see the node's infeasible count, not its own.
 *                   Without a communicator (one rank) it leaves buf unchanged.
 *   cmpc_comm_destroy: leaves the communicator (cmpc_destroy does it too).
 * ---------------------------------------------------------------------- */
#define CMPC_COMM_ID_BYTES 128
int cmpc_comm_id(unsigned char id[CMPC_COMM_ID_BYTES]);
int cmpc_comm_init(cmpc_ctx* ctx, int nranks, int rank, const unsigned char id[CMPC_COMM_ID_BYTES]);
int cmpc_allgather_trajectories(cmpc_ctx* ctx, const double* traj_local, double* traj_all, unsigned long long count,
                                void* hip_stream);
int cmpc_comm_sum_i32(cmpc_ctx* ctx, int* buf, unsigned long long count, void* hip_stream);
int cmpc_comm_destroy(cmpc_ctx* ctx);

/* Device self-test of the f64 MFMA fragment mapping used by the solver
 * (D = A*B for one 16x16x4 tile, A,B host 16x4 / 4x16 row-major, D host 16x16). */
int cmpc_selftest_mfma(cmpc_ctx* ctx, const double* A, const double* B, double* D);

/* Device self-test of the fused row-broadcast fma the v3 kernel uses (v_fmac_f64 with a DPP
 * row_newbcast source) against the two-instruction expression, on one wavefront.  A, X, C: host,
 * 64 doubles (one per lane).  fused, ref: host, [4][16][64] doubles: case, broadcast lane J, lane.
 * Cases: 0  fma(A, bcast_J(X), C);  1  fma(-bcast_J(X), A, C);  2  as 0 and 3  fma(-bcast_J(X), A, X),
 * both through the settled-source form.  The two arrays must be equal bit for bit. */
int cmpc_selftest_fma_bcast(cmpc_ctx* ctx, const double* A, const double* X, const double* C, double* fused,
                            double* ref);

#ifdef __cplusplus
}
#endif
#endif /* CMPC_H */
