"""The time-invariant instantiations' stage recursions with A and B held in registers (mpc_ipm3.hip, tr_on): psi3,
psi3seg, fwd3seg and fwd3 read the lane's row or column of stage 0 once per call and fetch only y_k or u_k per
stage; phi_build and psi_build read A once, and the table of the condensed dynamics' columns is kept in registers
until one store pass after its recursion (trb_on).  The same fmas on the same operands in the same order, so
DIRounds(lti=True) must give DIRounds(lti=False) (the per-stage fetches, untouched) bit for bit.

One step() of the fused round.  Besides z, kkt, iters and status the round's advance is compared: x0, u_prev and
traj_local come from the epilogue's forward recursion, which the older comparisons of the two paths leave out.
A converged solve hides a wrong direction, because the interior-point iteration corrects itself: the cases that
count stop after one and after two iterations.  The uncapped solve is compared as well.

Horizons (nu = 2, 16 columns per tile; the segmented recursions run from two tiles on, N > 8):
6, 7, 8 one tile, the serial fwd3 / psi3, all three remainders of their rotation by three | 9, 10, 11 two tiles,
the segmented forms with segments of unequal length (9: 3 2 2 2, 10: 3 2 3 2, 11: 3 3 3 2) | 17, 25 three and four
tiles with padding | 30 the workload's, 31 | 32 no padding column.  Neighbours 0 and 2.
The population is time-invariant with dense perturbed A and B (as test_v3_ti_frag_gpu.py's), so that no structural
zero of A or B can hide a wrong row, column or entry."""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZONS = [6, 7, 8, 9, 10, 11, 17, 25, 30, 31, 32]
NBS = [0, 2]
CAPS = [1, 2, None]   # max_iter: one Newton step, two, the solver's default
AGENTS = 40
EPS, SEED = 1e-2, 20240
OUT = ("z", "kkt", "iters", "status", "x0", "u_prev", "traj_local")


@functools.lru_cache(maxsize=None)
def scenario(N, nb):
    """make_di with every agent's A, B replaced by the integrator's plus EPS x a seeded dense normal matrix, the
    same at every stage."""
    from cmpc import scenarios as S

    sc = S.make_di(AGENTS, N, nb, 2)
    rng = np.random.default_rng(SEED)
    n, nx, nu = sc.n_agents, sc.A.shape[2], sc.B.shape[3]
    dA = EPS * rng.standard_normal((n, 1, nx, nx))
    dB = EPS * rng.standard_normal((n, 1, nx, nu))
    A = np.ascontiguousarray(np.broadcast_to(sc.A[:, :1] + dA, (n, N, nx, nx)))
    B = np.ascontiguousarray(np.broadcast_to(sc.B[:, :1] + dB, (n, N, nx, nu)))
    return dataclasses.replace(sc, A=A, B=B)


def one_round(gpu_ctx, sc, lti, cap):
    import torch
    from cmpc.rounds import DIRounds

    R = DIRounds(sc, ctx=gpu_ctx, lti=lti, max_iter=cap)
    R.step()
    torch.cuda.synchronize()
    return R, {a: getattr(R, a).detach().cpu().numpy().copy() for a in OUT}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("N", HORIZONS)
def test_registers_bit_equal_to_stage_fetches(gpu_ctx, N, nb, cap):
    from cmpc import _lib as L
    from cmpc.rounds import is_lti

    sc = scenario(N, nb)
    assert is_lti(sc.A, sc.B) and np.count_nonzero(sc.A[:, 0]) == sc.A[:, 0].size
    T, t = one_round(gpu_ctx, sc, True, cap)
    G, g = one_round(gpu_ctx, sc, False, cap)
    assert T.fused and G.fused
    assert T.opts.flags & L.CMPC_FLAG_LTI and not G.opts.flags & L.CMPC_FLAG_LTI
    assert np.isfinite(g["z"]).all()
    if cap is not None:
        # the cap binds: z is the iterate after exactly cap Newton steps
        assert (g["iters"] == cap).all(), g["iters"]
    for a in OUT:
        assert t[a].shape == g[a].shape and np.array_equal(t[a], g[a]), (a, int((t[a] != g[a]).sum()))
