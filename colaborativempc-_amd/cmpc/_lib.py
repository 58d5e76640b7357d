"""ctypes binding of libcmpc.so (include/cmpc.h).

The shared library is built in-tree (``colaborativempc-_amd/lib/libcmpc.so``) by
``__graft_entry__.build()`` / ``make -C colaborativempc-_amd/csrc``.  There is no
CPU fallback: if the library is missing, ``load()`` raises, and if no gfx950
device is present ``Context()`` raises ``CmpcError(CMPC_ERR_DEVICE)``.
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
# CMPC_LIB_PATH: an alternative build of the same ABI (profiling variants under tools/)
LIB_PATH = os.environ.get("CMPC_LIB_PATH") or os.path.join(ROOT, "lib", "libcmpc.so")
HEADER = os.path.join(os.path.dirname(ROOT), "include", "cmpc.h")

CMPC_OK = 0
CMPC_ERR_ARG = -1
CMPC_ERR_DEVICE = -2
CMPC_ERR_UNSUPPORTED = -3
CMPC_ERR_NOMEM = -4

CMPC_SOLVED = 1
CMPC_SOLVED_INACCURATE = 2
CMPC_MAX_ITER_REACHED = -2
CMPC_PRIMAL_INFEASIBLE = -3
CMPC_UNSOLVED = -10

STATUS_TEXT = {1: "solved", 2: "solved inaccurate", -2: "maximum iterations reached",
               -3: "primal infeasible", -10: "unsolved"}

_DP = ct.POINTER(ct.c_double)
_IP = ct.POINTER(ct.c_int)


CMPC_FLAG_GENERIC = 1
CMPC_FLAG_FP32 = 8
CMPC_FLAG_RICCATI = 16
CMPC_FLAG_RESCUE = 32   # Riccati continuation of agents whose condensed factorisation broke down
CMPC_FLAG_FINISH = 64   # ... also of breakdowns already at the rounding floor (status 2)
CMPC_FLAG_LANE = 128    # lane-per-agent stage-wise kernel, fp64
CMPC_FLAG_POLISH = 256  # with RESCUE: active-set polish of breakdowns at the rounding floor (OSQP polish=True)
CMPC_FLAG_ONE_WAVE = 512   # fused DS round: one wavefront per agent (the default)
CMPC_FLAG_TWO_WAVES = 1024  # ... two wavefronts per agent (opt-in: bit-identical, no faster at 512 agents)
CMPC_FLAG_LTI = 2048   # the caller's promise: A_k, B_k bit-equal to stage 0's at every stage, all finite (rounds.is_lti)
CMPC_FLAG_CERTIFY = 4096   # after the solve: status -3 for an agent with a verified Farkas ray (cmpc.infeas)
CMPC_CERT_TOL = 1e-9       # the certificate's threshold on (reach - h) / S
CMPC_FLAG_CERTIFY_ROWS = 8192   # with CERTIFY: then the combined-row certificate on the agents still short of 1, 2, -3
CMPC_CERT_ROWS_MAX_ITER = 512   # the combined-row certificate's iteration cap ...
CMPC_CERT_ROWS_CHECK_EVERY = 8  # ... and the iterations between two of its reachability checks
CMPC_FLAG_LPV = 16384       # the caller's promise: every agent holds the reference structure (structure.lpv_level >= 1)
CMPC_FLAG_LPV_AUTO = 32768  # host entries: the detector decides after the upload (cmpc_mpc_lpv_level_dev)
CMPC_FLAG_LPV_SPLIT = 65536  # every entry: the detector and a partition route each agent to its kernel on the device


def lpv_flags(lpv):
    """The flag bits of a wrapper's ``lpv`` argument: False: none; True: CMPC_FLAG_LPV (the caller's promise);
    "auto": CMPC_FLAG_LPV_AUTO (host-pointer entries: the library runs the detector first); "split":
    CMPC_FLAG_LPV_SPLIT (host and device entries: each agent goes to its kernel on the device, nothing is read
    back)."""
    if isinstance(lpv, str):
        if lpv == "split":
            return CMPC_FLAG_LPV_SPLIT
        if lpv != "auto":
            raise ValueError(f"lpv: True, False, 'auto' or 'split', not {lpv!r}")
        return CMPC_FLAG_LPV_AUTO
    return CMPC_FLAG_LPV if lpv else 0


def certify_flags(certify):
    """The flag bits of a wrapper's ``certify`` argument: False: none; True: CMPC_FLAG_CERTIFY (the single-row
    rule); "rows": CMPC_FLAG_CERTIFY_ROWS as well (then the combined-row rule on the agents it leaves)."""
    if isinstance(certify, str):
        if certify != "rows":
            raise ValueError(f"certify: True, False or 'rows', not {certify!r}")
        return CMPC_FLAG_CERTIFY | CMPC_FLAG_CERTIFY_ROWS
    return CMPC_FLAG_CERTIFY if certify else 0


class cmpc_opts(ct.Structure):
    _fields_ = [("tol", ct.c_double), ("max_iter", ct.c_int), ("flags", ct.c_int), ("stamps", ct.c_void_p),
                ("order", ct.c_void_p)]


class cmpc_mpc_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("nx", "nu", "N", "ns", "mc", "batch")]


class cmpc_mpc_weights(ct.Structure):
    _fields_ = [("Q", _DP), ("R", _DP), ("dR", _DP), ("Qs", _DP), ("u_ub", _DP), ("u_lb", _DP),
                ("row_slack", _IP), ("row_sign", _IP)]


CMPC_SOLVER_CONDENSED_V3, CMPC_SOLVER_CONDENSED, CMPC_SOLVER_RICCATI, CMPC_SOLVER_LANE = 1, 2, 3, 4


class cmpc_plan_info(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("solver", "lds_bytes", "wg_per_cu", "agents_per_wg", "waves_per_agent",
                                        "polish_lds_bytes", "polish_max_active")]


class cmpc_mpc_data(ct.Structure):
    _fields_ = [(k, _DP) for k in ("A", "B", "x0", "u_prev", "qlin", "C", "h")]


class cmpc_mpc_out(ct.Structure):
    _fields_ = [("z", _DP), ("kkt", _DP), ("iters", _IP), ("status", _IP)]


class cmpc_mpc_duals(ct.Structure):
    _fields_ = [("y", _DP), ("dua_res", _DP)]


class cmpc_mpc_cert(ct.Structure):
    _fields_ = [("ray", _DP), ("margin", _DP), ("row", _IP)]


class cmpc_mpc_cert_rows(ct.Structure):
    _fields_ = [("ray", _DP), ("margin", _DP), ("iters", _IP), ("nrows", _IP)]


class cmpc_lpv_params(ct.Structure):
    _fields_ = [(k, ct.c_double) for k in ("lf", "lr", "m", "I", "Cf", "Cr", "mu", "vx_ref", "min_dist",
                                           "max_vel", "min_vel", "max_rs", "max_ls", "max_ac", "max_dc",
                                           "dt", "wq")] + \
               [("Q", ct.c_double * 81), ("Qs", ct.c_double * 3), ("R", ct.c_double * 4), ("dR", ct.c_double * 4)]


class cmpc_track(ct.Structure):
    _fields_ = [("nseg", ct.c_int), ("s0", _DP), ("len", _DP), ("curv", _DP), ("half_width", _DP)]


class cmpc_lpv_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("batch", "N", "nb", "last_rows")]


class cmpc_lpv_data(ct.Structure):
    _fields_ = [(k, _DP) for k in ("x0", "x_last", "u_last", "u_old", "x_agents", "pose")]


class cmpc_lpv_out(ct.Structure):
    _fields_ = [("z", _DP), ("planes", _DP), ("kkt", _DP), ("iters", _IP), ("status", _IP)]


class cmpc_lpv_build_out(ct.Structure):
    _fields_ = [("A", _DP), ("B", _DP), ("qlin", _DP), ("C", _DP), ("h", _DP), ("planes", _DP), ("err", _IP)]


class cmpc_di_params(ct.Structure):
    _fields_ = [("dim", ct.c_int)] + [(k, ct.c_double) for k in ("v_ref", "q_v", "q_lane", "hw", "min_vel",
                                                                 "max_vel", "min_dist", "wq")]


class cmpc_di_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("batch", "N", "nb", "self_offset")]


class cmpc_nbr_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("batch", "N", "nb", "self_offset", "n_total", "k0", "k1")]


CMPC_ROUNDS_HOST_EXCHANGE = 1
CMPC_ROUNDS_NO_HALT = 2
CMPC_ROUNDS_RESELECT = 4   # every round starts with the (0, 0) neighbour selection on the exchange buffer


class cmpc_lpv_rounds_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("n_total", "batch", "self_offset", "N", "nb", "flags")]


class cmpc_lpv_rounds_init(ct.Structure):
    _fields_ = [("x0", _DP), ("x_last", _DP), ("u_last", _DP), ("u_old", _DP), ("nbr", _IP), ("traj", _DP)]


class cmpc_lpv_rounds_out(ct.Structure):
    _fields_ = [("z", _DP), ("kkt", _DP), ("iters", _IP), ("status", _IP), ("x0", _DP), ("planes", _DP)]


CMPC_ROUNDS_LPT = 8        # cmpc_di_rounds / cmpc_lin_rounds: launch order = cmpc_order_by_iters_dev of the previous round's iterations


class cmpc_di_rounds_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("n_total", "batch", "self_offset", "N", "nb", "flags", "history")]


class cmpc_di_rounds_init(ct.Structure):
    _fields_ = [("A", _DP), ("B", _DP), ("x0", _DP), ("u_prev", _DP), ("lane", _DP), ("nbr", _IP), ("traj", _DP)]


class cmpc_di_rounds_out(ct.Structure):
    _fields_ = [("z", _DP), ("kkt", _DP), ("iters", _IP), ("status", _IP), ("x0", _DP), ("u_prev", _DP), ("nbr", _IP)]


class cmpc_lin_params(ct.Structure):   # position = state columns ix, iy
    _fields_ = [("ix", ct.c_int), ("iy", ct.c_int), ("min_dist", ct.c_double), ("wq", ct.c_double)]


class cmpc_lin3_params(ct.Structure):  # position = state columns ix, iy, iz (cmpc_lin3_*)
    _fields_ = [("ix", ct.c_int), ("iy", ct.c_int), ("iz", ct.c_int), ("min_dist", ct.c_double), ("wq", ct.c_double)]


class cmpc_lin_dims(ct.Structure):     # mo own rows per stage; mc = mo + nb
    _fields_ = [(k, ct.c_int) for k in ("batch", "N", "nb", "self_offset", "nx", "mo")]


class cmpc_lin_own(ct.Structure):      # device pointers
    _fields_ = [("qlin_own", _DP), ("C_own", _DP), ("h_own", _DP)]


class cmpc_lin_rounds_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("n_total", "batch", "self_offset", "N", "nb", "flags", "history", "nx", "nu",
                                        "ns", "mo")]


class cmpc_lin_rounds_init(ct.Structure):
    _fields_ = [("A", _DP), ("B", _DP), ("x0", _DP), ("u_prev", _DP), ("qlin_own", _DP), ("C_own", _DP),
                ("h_own", _DP), ("nbr", _IP), ("traj", _DP)]


class cmpc_lin_rounds_out(ct.Structure):
    _fields_ = [("z", _DP), ("kkt", _DP), ("iters", _IP), ("status", _IP), ("x0", _DP), ("u_prev", _DP), ("nbr", _IP)]


CMPC_TABLE_HOLD = 0        # a stage table past its end holds its last stage
CMPC_TABLE_PERIODIC = 1    # row(tau) = tau mod T


class cmpc_lin_table_dims(ct.Structure):
    _fields_ = [("T", ct.c_int), ("mode", ct.c_int)]


class cmpc_lin_table(ct.Structure):    # device pointers (cmpc_lin_rounds_table_write: host pointers)
    _fields_ = [("A", _DP), ("B", _DP), ("qlin", _DP), ("C", _DP), ("h", _DP)]


class cmpc_lin_rounds_table_init(ct.Structure):
    _fields_ = [("T", ct.c_int), ("mode", ct.c_int), ("t0", ct.c_int), ("A", _DP), ("B", _DP), ("qlin", _DP),
                ("C", _DP), ("h", _DP), ("x0", _DP), ("u_prev", _DP), ("nbr", _IP), ("traj", _DP)]


class cmpc_consensus_opts(ct.Structure):   # the stopping rule of a consensus step (scenarios.consensus_stop)
    _fields_ = [("min_rounds", ct.c_int), ("need", ct.c_int), ("max_rounds", ct.c_int), ("atol", ct.c_double),
                ("rtol", ct.c_double)]


class cmpc_consensus_out(ct.Structure):    # host pointers, any may be None
    _fields_ = [("inner_rounds", _IP), ("agreed", _IP), ("not_close", _IP), ("cap", ct.c_int), ("close", _IP),
                ("delta", _DP)]


class cmpc_log_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("batch", "nx", "nu", "ns", "N", "look_col")]


class cmpc_log_row(ct.Structure):   # device pointers to one round's rows
    _fields_ = [("state", _DP), ("u", _DP), ("look_ahead", _DP), ("kkt", _DP), ("iters", _IP), ("status", _IP)]


CMPC_LOG_SEPARATION = 1    # the log also keeps each agent's nearest other agent and the squared distance


class cmpc_rounds_log(ct.Structure):   # host pointers, leading dimension = count
    _fields_ = [("state", _DP), ("u", _DP), ("look_ahead", _DP), ("kkt", _DP), ("iters", _IP), ("status", _IP),
                ("sep2", _DP), ("nearest", _IP), ("solve_ms", _DP)]


class cmpc_qp_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("n", "m_ineq", "m_eq", "batch", "col_major")]


class cmpc_qp_data(ct.Structure):
    _fields_ = [(k, _DP) for k in ("H", "f", "A", "b", "Aeq", "beq", "lb", "ub")]


class cmpc_qp_out(ct.Structure):
    _fields_ = [("x", _DP), ("fval", _DP), ("exitflag", _IP), ("iters", _IP), ("lambda_ineqlin", _DP),
                ("lambda_eqlin", _DP), ("lambda_lower", _DP), ("lambda_upper", _DP), ("residual", _DP)]


CMPC_QP_CONVERGED = 1
CMPC_QP_MAXITER = 0
CMPC_QP_INFEASIBLE = -2
CMPC_QP_UNBOUNDED = -3
CMPC_QP_NONCONVEX = -6


class cmpc_ocd_dims(ct.Structure):
    _fields_ = [(k, ct.c_int) for k in ("batch", "N", "nb", "self_offset")]


class CmpcError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"libcmpc error {code}: {msg}")
        self.code = code


_LIB = None

# name -> (restype, argtypes) for every function declared in include/cmpc.h
SIGNATURES = {
    "cmpc_abi_version": (ct.c_int, []),
    "cmpc_create": (ct.c_int, [ct.POINTER(ct.c_void_p), ct.c_int]),
    "cmpc_destroy": (ct.c_int, [ct.c_void_p]),
    "cmpc_last_error": (ct.c_char_p, [ct.c_void_p]),
    "cmpc_solve_mpc_batch": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                        ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out), ct.POINTER(cmpc_opts)]),
    "cmpc_solve_mpc_batch_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                            ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out),
                                            ct.POINTER(cmpc_opts), ct.c_void_p]),
    "cmpc_solve_mpc_batch_duals": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                              ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out),
                                              ct.POINTER(cmpc_mpc_duals), ct.POINTER(cmpc_opts)]),
    "cmpc_solve_mpc_batch_duals_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims),
                                                  ct.POINTER(cmpc_mpc_weights), ct.POINTER(cmpc_mpc_data),
                                                  ct.POINTER(cmpc_mpc_out), ct.POINTER(cmpc_mpc_duals),
                                                  ct.POINTER(cmpc_opts), ct.c_void_p]),
    "cmpc_mpc_duals_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                      ct.POINTER(cmpc_mpc_data), _DP, _DP, ct.POINTER(cmpc_mpc_duals), ct.c_void_p]),
    "cmpc_mpc_certify": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                    ct.POINTER(cmpc_mpc_data), _IP, ct.POINTER(cmpc_mpc_cert)]),
    "cmpc_mpc_certify_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                        ct.POINTER(cmpc_mpc_data), _IP, ct.POINTER(cmpc_mpc_cert), ct.c_void_p]),
    "cmpc_mpc_certify_rows": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                         ct.POINTER(cmpc_mpc_data), _IP, ct.POINTER(cmpc_mpc_cert_rows), ct.c_int,
                                         ct.c_int]),
    "cmpc_mpc_certify_rows_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                             ct.POINTER(cmpc_mpc_data), _IP, ct.POINTER(cmpc_mpc_cert_rows),
                                             ct.c_int, ct.c_int, ct.c_void_p]),
    "cmpc_mpc_lpv_level": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                      ct.POINTER(cmpc_mpc_data), _IP, _IP]),
    "cmpc_mpc_lpv_level_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                          ct.POINTER(cmpc_mpc_data), _IP, _IP, ct.c_void_p]),
    "cmpc_mpc_lpv_split_dev": (ct.c_int, [ct.c_void_p, ct.c_int, _IP, _IP, _IP, ct.c_void_p]),
    "cmpc_solve_lpv_batch": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lpv_params), ct.POINTER(cmpc_track),
                                        ct.POINTER(cmpc_lpv_dims), ct.POINTER(cmpc_lpv_data),
                                        ct.POINTER(cmpc_lpv_out), ct.POINTER(cmpc_opts)]),
    "cmpc_solve_lpv_batch_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lpv_params), ct.POINTER(cmpc_track),
                                            ct.POINTER(cmpc_lpv_dims), ct.POINTER(cmpc_lpv_data),
                                            ct.POINTER(cmpc_lpv_out), ct.POINTER(cmpc_opts), ct.c_void_p]),
    "cmpc_di_build_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_params), ct.POINTER(cmpc_di_dims),
                                     _IP, _DP, _DP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_di_solve_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_params), ct.POINTER(cmpc_di_dims), _IP, _DP,
                                     _DP, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                     ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out), ct.POINTER(cmpc_opts),
                                     ct.c_void_p]),
    "cmpc_di_round_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_params), ct.POINTER(cmpc_di_dims), _IP, _DP,
                                     _DP, ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                     ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out), ct.POINTER(cmpc_opts),
                                     _DP, ct.c_void_p]),
    "cmpc_lpv_gather_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_dims), _IP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_nbr_select_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_nbr_dims), _DP, _IP, _DP, ct.c_void_p]),
    "cmpc_lpv_advance_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_dims), _DP, _DP, _DP, _DP, _DP, _DP,
                                        _IP, _IP, ct.c_void_p]),
    "cmpc_di_advance_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_params), ct.POINTER(cmpc_di_dims),
                                       _DP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_solve_qp_batch": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_qp_dims), ct.POINTER(cmpc_qp_data),
                                       ct.POINTER(cmpc_qp_out), ct.POINTER(cmpc_opts)]),
    "cmpc_ocd_update_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_ocd_dims), ct.c_double, ct.c_double, _IP, _DP,
                                       _DP, ct.c_void_p]),
    "cmpc_ocd_converged_dev": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, ct.c_double, ct.c_double, _DP, _DP, _IP,
                                          ct.c_void_p]),
    "cmpc_selftest_mfma": (ct.c_int, [ct.c_void_p, _DP, _DP, _DP]),
    "cmpc_selftest_fma_bcast": (ct.c_int, [ct.c_void_p, _DP, _DP, _DP, _DP, _DP]),
    "cmpc_lpv_build_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lpv_params), ct.POINTER(cmpc_track),
                                      ct.POINTER(cmpc_lpv_dims), ct.POINTER(cmpc_lpv_data),
                                      ct.POINTER(cmpc_lpv_build_out), ct.c_void_p]),
    "cmpc_comm_id": (ct.c_int, [ct.c_char_p]),
    "cmpc_comm_init": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, ct.c_char_p]),
    "cmpc_allgather_trajectories": (ct.c_int, [ct.c_void_p, _DP, _DP, ct.c_ulonglong, ct.c_void_p]),
    "cmpc_comm_sum_i32": (ct.c_int, [ct.c_void_p, _IP, ct.c_ulonglong, ct.c_void_p]),
    "cmpc_plan_mpc": (ct.c_int, [ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights), ct.POINTER(cmpc_opts),
                                 ct.POINTER(cmpc_plan_info)]),
    "cmpc_comm_destroy": (ct.c_int, [ct.c_void_p]),
    "cmpc_lpv_rounds_create": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lpv_params), ct.POINTER(cmpc_track),
                                          ct.POINTER(cmpc_lpv_rounds_dims), ct.POINTER(cmpc_lpv_rounds_init),
                                          ct.POINTER(cmpc_opts), ct.POINTER(ct.c_void_p)]),
    "cmpc_lpv_rounds_step": (ct.c_int, [ct.c_void_p, ct.c_int, _IP, _IP]),
    "cmpc_lpv_rounds_read": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lpv_rounds_out)]),
    "cmpc_lpv_rounds_get_traj": (ct.c_int, [ct.c_void_p, _DP]),
    "cmpc_lpv_rounds_set_traj": (ct.c_int, [ct.c_void_p, _DP]),
    "cmpc_lpv_rounds_destroy": (ct.c_int, [ct.c_void_p]),
    "cmpc_order_by_iters_dev": (ct.c_int, [ct.c_void_p, ct.c_int, _IP, _IP, ct.c_void_p]),
    "cmpc_di_rounds_create": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_params), ct.POINTER(cmpc_mpc_weights),
                                         ct.POINTER(cmpc_di_rounds_dims), ct.POINTER(cmpc_di_rounds_init),
                                         ct.POINTER(cmpc_opts), ct.POINTER(ct.c_void_p)]),
    "cmpc_di_rounds_step": (ct.c_int, [ct.c_void_p, ct.c_int, _IP]),
    "cmpc_di_rounds_read": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_rounds_out)]),
    "cmpc_di_rounds_history": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, _DP, _IP, _IP]),
    "cmpc_di_rounds_get_traj": (ct.c_int, [ct.c_void_p, _DP]),
    "cmpc_di_rounds_set_traj": (ct.c_int, [ct.c_void_p, _DP]),
    "cmpc_di_rounds_destroy": (ct.c_int, [ct.c_void_p]),
    "cmpc_round_log_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_log_dims), _DP, _DP, _IP, _IP,
                                      ct.POINTER(cmpc_log_row), ct.c_void_p]),
    "cmpc_lpv_rounds_log_enable": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int]),
    "cmpc_lpv_rounds_log_range": (ct.c_int, [ct.c_void_p, _IP, _IP]),
    "cmpc_lpv_rounds_log_read": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, ct.POINTER(cmpc_rounds_log)]),
    "cmpc_di_rounds_log_enable": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int]),
    "cmpc_di_rounds_log_range": (ct.c_int, [ct.c_void_p, _IP, _IP]),
    "cmpc_di_rounds_log_read": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, ct.POINTER(cmpc_rounds_log)]),
    "cmpc_lin_build_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_params), ct.POINTER(cmpc_lin_dims), _IP,
                                      ct.POINTER(cmpc_lin_own), _DP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_lin_advance_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_params), ct.POINTER(cmpc_lin_dims), ct.c_int,
                                        ct.c_int, _DP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_lin_round_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_params), ct.POINTER(cmpc_lin_dims), _IP,
                                      ct.POINTER(cmpc_lin_own), _DP, ct.POINTER(cmpc_mpc_dims),
                                      ct.POINTER(cmpc_mpc_weights), ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out),
                                      ct.POINTER(cmpc_opts), _DP, ct.c_void_p]),
    "cmpc_lin_rounds_create": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_params), ct.POINTER(cmpc_mpc_weights),
                                          ct.POINTER(cmpc_lin_rounds_dims), ct.POINTER(cmpc_lin_rounds_init),
                                          ct.POINTER(cmpc_opts), ct.POINTER(ct.c_void_p)]),
    "cmpc_lin_rounds_step": (ct.c_int, [ct.c_void_p, ct.c_int, _IP]),
    "cmpc_lin_rounds_read": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_rounds_out)]),
    "cmpc_lin_rounds_history": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, _DP, _IP, _IP]),
    "cmpc_lin_rounds_get_traj": (ct.c_int, [ct.c_void_p, _DP]),
    "cmpc_lin_rounds_set_traj": (ct.c_int, [ct.c_void_p, _DP]),
    "cmpc_lin_rounds_set_state": (ct.c_int, [ct.c_void_p, _DP, _DP]),
    "cmpc_lin_rounds_destroy": (ct.c_int, [ct.c_void_p]),
    "cmpc_lin_rounds_log_enable": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int]),
    "cmpc_lin_rounds_log_range": (ct.c_int, [ct.c_void_p, _IP, _IP]),
    "cmpc_lin_rounds_log_read": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, ct.POINTER(cmpc_rounds_log)]),
    "cmpc_lin_table_build_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_params), ct.POINTER(cmpc_lin_dims), ct.c_int,
                                            ct.POINTER(cmpc_lin_table_dims), ct.POINTER(cmpc_lin_table), ct.c_int, _IP,
                                            _DP, _DP, _DP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_lin_table_round_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_params), ct.POINTER(cmpc_lin_dims), _IP,
                                            ct.POINTER(cmpc_lin_table_dims), ct.POINTER(cmpc_lin_table), ct.c_int, _DP,
                                            ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                            ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out), ct.POINTER(cmpc_opts),
                                            _DP, ct.c_void_p]),
    "cmpc_lin_rounds_create_table": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_params), ct.POINTER(cmpc_mpc_weights),
                                                ct.POINTER(cmpc_lin_rounds_dims),
                                                ct.POINTER(cmpc_lin_rounds_table_init), ct.POINTER(cmpc_opts),
                                                ct.POINTER(ct.c_void_p)]),
    "cmpc_lin_rounds_get_time": (ct.c_int, [ct.c_void_p, _IP]),
    "cmpc_lin_rounds_set_time": (ct.c_int, [ct.c_void_p, ct.c_int]),
    "cmpc_lin_rounds_table_write": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, ct.POINTER(cmpc_lin_table)]),
    "cmpc_lin_publish_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin_params), ct.POINTER(cmpc_lin_dims), ct.c_int,
                                        ct.c_int, _DP, _DP, ct.c_double, ct.c_double, _DP, _IP, _DP, _IP, ct.c_void_p]),
    "cmpc_lin_rounds_step_consensus": (ct.c_int, [ct.c_void_p, ct.c_int, ct.POINTER(cmpc_consensus_opts), _IP, _IP]),
    "cmpc_lin_rounds_consensus_read": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_consensus_out)]),
    "cmpc_lpv_publish_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_di_dims), _DP, _DP, _IP, ct.c_double, ct.c_double,
                                        _DP, _IP, _DP, _IP, ct.c_void_p]),
    "cmpc_lpv_rounds_step_consensus": (ct.c_int, [ct.c_void_p, ct.c_int, ct.POINTER(cmpc_consensus_opts), _IP, _IP,
                                                  _IP]),
    "cmpc_lpv_rounds_consensus_read": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_consensus_out)]),
    "cmpc_lin3_build_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin3_params), ct.POINTER(cmpc_lin_dims), _IP,
                                       ct.POINTER(cmpc_lin_own), _DP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_lin3_advance_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin3_params), ct.POINTER(cmpc_lin_dims), ct.c_int,
                                         ct.c_int, _DP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_lin3_publish_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin3_params), ct.POINTER(cmpc_lin_dims), ct.c_int,
                                         ct.c_int, _DP, _DP, ct.c_double, ct.c_double, _DP, _IP, _DP, _IP, ct.c_void_p]),
    "cmpc_lin3_round_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin3_params), ct.POINTER(cmpc_lin_dims), _IP,
                                       ct.POINTER(cmpc_lin_own), _DP, ct.POINTER(cmpc_mpc_dims),
                                       ct.POINTER(cmpc_mpc_weights), ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out),
                                       ct.POINTER(cmpc_opts), _DP, ct.c_void_p]),
    "cmpc_lin3_table_build_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin3_params), ct.POINTER(cmpc_lin_dims),
                                             ct.c_int, ct.POINTER(cmpc_lin_table_dims), ct.POINTER(cmpc_lin_table),
                                             ct.c_int, _IP, _DP, _DP, _DP, _DP, _DP, _DP, ct.c_void_p]),
    "cmpc_lin3_table_round_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin3_params), ct.POINTER(cmpc_lin_dims), _IP,
                                             ct.POINTER(cmpc_lin_table_dims), ct.POINTER(cmpc_lin_table), ct.c_int, _DP,
                                             ct.POINTER(cmpc_mpc_dims), ct.POINTER(cmpc_mpc_weights),
                                             ct.POINTER(cmpc_mpc_data), ct.POINTER(cmpc_mpc_out), ct.POINTER(cmpc_opts),
                                             _DP, ct.c_void_p]),
    "cmpc_nbr_select3_dev": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_nbr_dims), _DP, _IP, _DP, ct.c_void_p]),
    "cmpc_lin_rounds_create3": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin3_params), ct.POINTER(cmpc_mpc_weights),
                                           ct.POINTER(cmpc_lin_rounds_dims), ct.POINTER(cmpc_lin_rounds_init),
                                           ct.POINTER(cmpc_opts), ct.POINTER(ct.c_void_p)]),
    "cmpc_lin_rounds_create_table3": (ct.c_int, [ct.c_void_p, ct.POINTER(cmpc_lin3_params), ct.POINTER(cmpc_mpc_weights),
                                                 ct.POINTER(cmpc_lin_rounds_dims),
                                                 ct.POINTER(cmpc_lin_rounds_table_init), ct.POINTER(cmpc_opts),
                                                 ct.POINTER(ct.c_void_p)]),
    "cmpc_lin_rounds_pos_dim": (ct.c_int, [ct.c_void_p, _IP]),
}

CMPC_COMM_ID_BYTES = 128


def load():
    """Load libcmpc.so (raises FileNotFoundError if it was not built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run __graft_entry__.build() "
                                    f"or make -C colaborativempc-_amd/csrc")
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (SONAME
        # libamdhip64.so.7) and loads it by the unversioned name.  Loading torch first
        # makes libcmpc's NEEDED libamdhip64.so.7 bind to that same runtime; loading
        # libcmpc first would give the process two runtimes and torch would see no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ct.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def dptr(a):
    return None if a is None else a.ctypes.data_as(_DP)


def iptr(a):
    return None if a is None else a.ctypes.data_as(_IP)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def opts(tol=None, max_iter=None, flags=0, stamps=None, order=None):
    """cmpc_opts; stamps / order: device pointers (int) or None."""
    return cmpc_opts(float(tol or 0.0), int(max_iter or 0), int(flags), stamps, order)


class Context:
    """One libcmpc context on one HIP device (cmpc_create / cmpc_destroy)."""

    def __init__(self, device=0):
        self.lib = load()
        h = ct.c_void_p()
        rc = self.lib.cmpc_create(ct.byref(h), int(device))
        if rc != CMPC_OK:
            raise CmpcError(rc, f"cmpc_create(device={device}) failed: no usable gfx950 device")
        self.h = h
        self.device = device

    def check(self, rc):
        if rc != CMPC_OK:
            msg = self.lib.cmpc_last_error(self.h)
            raise CmpcError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "h", None):
            self.lib.cmpc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT = {}


def default_context(device=0):
    if device not in _DEFAULT:
        _DEFAULT[device] = Context(device)
    return _DEFAULT[device]
