"""The v3 kernel's second pass over its instruction overhead (mpc_ipm3.hip; DESIGN.md §3, "second census pass"):
theta, 1 / t and 1 / D_sigma formed once per iteration and held across the factorisation (theta_once), and the K
build's diagonal adds read through indices the lane forms once per solve (dg_addr_on).  Both keep every operation,
operand and order, so nothing may change by a bit.

The two-tile instantiations (N = 9 .. 16) have neither form and compile to the parent's instruction stream: with
either compiled in, [16-1] (and with both, [16-2]) failed here from the second iteration on (the first equal; max
|dz| 0.072 on all five agents), while the parent passed all 28 cases; the signature of the two-tile defect that
tf_on records (mpc_ipm3.hip), whose cause is not found.

Two consecutive rounds of DIRounds(fused=True), the structured DS / TI instantiations with the rows built in the
launch, against DIRounds(fused=False), the dense instantiation behind di_build_kernel, with and without the
time-invariance promise, stopped after one and after two iterations (z is then one or two Newton steps: a converged
solve would correct a wrong K or a wrong theta by itself) and uncapped.  z, kkt, iters, status and the exchanged
x0, u_prev, traj_all are compared as 64-bit patterns.

Horizons (nu = 2, 16 columns per tile): 7 one tile with padding | 8 one full tile | 9 the two-tile instantiation |
16, 17 | 24 three full tiles and 23 < n / 2 <= 24, run by the four-tile instantiation (mpc3_tiles) | 25 four tiles
with padding | 30 the workload's | 32 no padding column.  Neighbours 0, 1, 2.  Five agents: not a multiple of the
four per CU.

One case (N = 30, nb = 2) has u_lb = -inf on one input: a row of the input lanes that exists but has no finite
bound, so lanes without an active row take the select arms.  The C restatement ends every agent of it at status 1
(checked here on the CPU), and the fused round must match it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZONS = [7, 8, 9, 16, 17, 24, 25, 30, 32]
NBS = [0, 1, 2]
CAPS = [1, 2, None]   # max_iter: one Newton step, two, the solver's default
AGENTS = 5
ROUNDS = 2
OUT = ("z", "kkt", "iters", "status", "x0", "u_prev", "traj_all")
Z_TOL = 1e-6          # test_gpu.test_synthetic_batch_vs_c_oracle


def _scenario(N, nb, inf_lb=False):
    from cmpc import scenarios as S

    sc = S.make_di(AGENTS, N, nb, 2)
    if inf_lb:
        sc.shared["u_lb"] = np.array([sc.shared["u_lb"][0], -np.inf])
    return sc


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _rounds_equal(gpu_ctx, sc, lti, cap):
    """ROUNDS consecutive rounds, fused against build-then-solve; returns the fused handle's first-round z / status."""
    import torch
    from cmpc.rounds import DIRounds

    F = DIRounds(sc, ctx=gpu_ctx, fused=True, lti=lti, max_iter=cap)
    U = DIRounds(sc, ctx=gpu_ctx, fused=False, lti=lti, max_iter=cap)
    first = None
    for rnd in range(ROUNDS):
        F.step()
        U.step()
        torch.cuda.synchronize()
        f = {a: getattr(F, a).detach().cpu().numpy().copy() for a in OUT}
        u = {a: getattr(U, a).detach().cpu().numpy().copy() for a in OUT}
        assert np.isfinite(u["z"]).all(), (lti, cap, rnd)
        if cap is not None:
            assert (u["iters"] == cap).all(), (lti, cap, rnd, u["iters"])   # the cap binds
        for a in OUT:
            fb, ub = _bits(f[a]), _bits(u[a])
            assert fb.shape == ub.shape and np.array_equal(fb, ub), (lti, cap, rnd, a, int((fb != ub).sum()))
        first = first or f
    return first


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("N", HORIZONS)
def test_fused_rounds_bit_equal_to_build_then_solve(gpu_ctx, N, nb):
    sc = _scenario(N, nb)
    for lti in (True, False):
        for cap in CAPS:
            _rounds_equal(gpu_ctx, sc, lti, cap)


@functools.lru_cache(maxsize=None)
def _reference_inf_lb():
    """The C restatement's solution of the unbounded-input case (computed once, read-only)."""
    from oracle import cmpc_oracle as CO
    from oracle import synth

    sc = _scenario(30, 2, True)
    P = synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj,
                         np.arange(AGENTS))
    z, _, _, st = CO.solve_batch(P)
    z.setflags(write=False)
    st.setflags(write=False)
    return z, st


def test_rows_without_a_finite_bound(gpu_ctx):
    import cmpc

    zc, stc = _reference_inf_lb()
    assert (stc == 1).all(), stc
    sc = _scenario(30, 2, True)
    for lti in (True, False):
        for cap in CAPS:
            f = _rounds_equal(gpu_ctx, sc, lti, cap)
            if cap is None:
                assert (f["status"] == cmpc.CMPC_SOLVED).all(), (lti, f["status"])
                assert np.abs(f["z"] - zc).max() < Z_TOL, (lti, float(np.abs(f["z"] - zc).max()))
