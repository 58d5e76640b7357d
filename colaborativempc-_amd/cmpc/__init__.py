"""cmpc — MI355X-native batched collaborative-MPC QP solver (host side).

The compute path is libcmpc.so (HIP kernels for gfx950 behind the C ABI in
include/cmpc.h).  This package is the host-side mirror of the reference's
planner interface (MarcFacerias/ColaborativeMPC-, planner/lib/plan_lib) plus the
round driver and synthetic workloads.  There is no CPU solve path here.
"""
from . import duals, infeas
from ._lib import (CMPC_MAX_ITER_REACHED, CMPC_PRIMAL_INFEASIBLE, CMPC_SOLVED, CMPC_SOLVED_INACCURATE, CMPC_UNSOLVED,
                   CmpcError, Context, default_context, load)
from .planner import PlannerLPV, PlannerLPVBatch, feasible_of, unpack
from .qp import osqp_solve_qp, osqp_solve_qp_batch, quadprog
from .rounds import (DIRoundsHandle, LinRoundsHandle, LinTableRoundsHandle, log_round_dev, order_by_iters_dev,
                     select_neighbours_dev)
from .scenarios import (lin_advance, lin_of_di, lin_rows, lin_table_of_di, lin_table_rows, lin_window, log_row,
                        order_by_iters, select_neighbours)
from .solver import nz_of, selftest_fma_bcast, selftest_mfma, solve_mpc, solve_mpc_dev

__all__ = ["duals", "infeas", "CMPC_PRIMAL_INFEASIBLE", "log_row", "log_round_dev", "select_neighbours", "select_neighbours_dev", "order_by_iters", "order_by_iters_dev", "DIRoundsHandle",
           "LinRoundsHandle", "lin_rows", "lin_advance", "lin_of_di",
           "LinTableRoundsHandle", "lin_table_rows", "lin_window", "lin_table_of_di",
           "Context", "CmpcError", "default_context", "load", "PlannerLPV", "PlannerLPVBatch", "feasible_of",
           "unpack", "quadprog", "osqp_solve_qp", "osqp_solve_qp_batch", "solve_mpc", "solve_mpc_dev", "nz_of", "selftest_mfma", "selftest_fma_bcast", "CMPC_SOLVED",
           "CMPC_SOLVED_INACCURATE", "CMPC_MAX_ITER_REACHED", "CMPC_UNSOLVED"]
