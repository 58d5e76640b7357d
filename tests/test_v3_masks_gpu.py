"""The v3 kernel's lane masks at the shapes where they change: stage lanes that own no stage (k >= N),
input lanes past n = N nu, padding columns n .. 16 T - 1, and the tile-count boundaries.

Batches of 3 agents of the 2-D double integrator at (N, nb) with T = 2, 2, 2, 3, 3, 4, 4 tiles (N = 9: the
shortest horizon with the segmented recursions; N = 32: no idle stage lane), each solved by
  * the fused round (cmpc_di_solve_dev: the structured DS instantiation),
  * build-then-solve (cmpc_di_build_dev + cmpc_solve_mpc_batch_dev: the dense v3 instantiation),
  * the runtime-dimension kernel (CMPC_FLAG_GENERIC).
The first two must agree bit for bit; all three must match the C restatement of the method
(oracle.cmpc_oracle.solve_batch) within the bars of test_gpu.test_synthetic_batch_vs_c_oracle.  One case has
u_lb = -inf on one input (a row of the lane that exists but is inactive), one stops at max_iter = 3 (the
best-iterate restore).  The C restatement ends every uncapped case at status 1 (checked on the CPU), so no
case is skipped.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Z_TOL = 1e-6   # test_gpu.test_synthetic_batch_vs_c_oracle
KKT_TOL = 1e-6
N_AGENTS = 3

# (N, nb, u_lb = -inf on input 1, max_iter (0: the default))
CASES = [(9, 0, False, 0), (9, 2, False, 0), (16, 1, False, 0), (17, 2, False, 0), (24, 2, False, 0),
         (30, 2, False, 0), (32, 2, False, 0), (30, 2, True, 0), (17, 2, False, 3)]


def _scenario(N, nb, inf_lb):
    from cmpc import scenarios as S

    sc = S.make_di(N_AGENTS, N, nb, 2)
    if inf_lb:
        sc.shared["u_lb"] = np.array([sc.shared["u_lb"][0], -np.inf])
    return sc


@functools.lru_cache(maxsize=None)
def _reference(N, nb, inf_lb, cap):
    """The C restatement's solution of the case (computed once, read-only)."""
    from oracle import cmpc_oracle as CO
    from oracle import synth

    sc = _scenario(N, nb, inf_lb)
    P = synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj,
                         np.arange(N_AGENTS))
    z, kkt, it, st = CO.solve_batch(P, max_iter=cap or 60)
    for a in (z, kkt, it, st):
        a.setflags(write=False)
    return z, kkt, it, st


def _solve(gpu_ctx, sc, path, cap):
    import torch
    from cmpc import _lib as L
    from cmpc.rounds import DIRounds

    R = DIRounds(sc, ctx=gpu_ctx, max_iter=cap or None)
    if path == "generic":
        R.opts = L.opts(None, cap or None, L.CMPC_FLAG_GENERIC)
    if path == "fused":
        R.build_solve()
    else:
        R.build()
        R.solve()
    torch.cuda.synchronize()
    return {k: getattr(R, k).cpu().numpy() for k in ("z", "kkt", "iters", "status")}


@pytest.mark.parametrize("N,nb,inf_lb,cap", CASES)
def test_v3_masks_three_paths(gpu_ctx, N, nb, inf_lb, cap):
    import cmpc

    sc = _scenario(N, nb, inf_lb)
    zc, kc, ic, stc = _reference(N, nb, inf_lb, cap)
    if not cap:
        assert (stc == 1).all(), stc   # nothing below is conditional on the reference's status
    res = {p: _solve(gpu_ctx, sc, p, cap) for p in ("fused", "dense", "generic")}
    for p, r in res.items():
        print(f"N {N} nb {nb} inf_lb {inf_lb} max_iter {cap or 'default'} {p}: status {r['status'].tolist()} iters "
              f"{r['iters'].tolist()} kkt {r['kkt'].max():.2e} max|z - z_c| {np.abs(r['z'] - zc).max():.2e}")
    for k in ("z", "kkt", "iters", "status"):
        np.testing.assert_array_equal(res["fused"][k], res["dense"][k], err_msg=f"fused vs dense v3: {k}")
    for p, r in res.items():
        if cap:   # stopped at the cap on both sides: the restored best iterate
            np.testing.assert_array_equal(r["status"], stc, err_msg=p)
            np.testing.assert_array_equal(r["iters"], ic, err_msg=p)
        else:
            assert np.isin(r["status"], (cmpc.CMPC_SOLVED, cmpc.CMPC_SOLVED_INACCURATE)).all(), (p, r["status"])
            assert (r["status"] == cmpc.CMPC_SOLVED).mean() > 0.99, (p, r["status"])
            assert r["kkt"].max() < KKT_TOL, (p, r["kkt"].max())
        assert np.abs(r["z"] - zc).max() < Z_TOL, (p, np.abs(r["z"] - zc).max())
