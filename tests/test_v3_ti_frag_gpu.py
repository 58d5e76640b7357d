"""The time-invariant K build's MFMA fragments formed in place (mpc_ipm3.hip, tf_on): lane (l & 15, l >> 4) reads
its entries of Gamma and of W Gamma from the table's and the stage weights' fragment images instead of receiving
them by a row transpose.  The same fmas on the same operands, so DIRounds(lti=True) must give DIRounds(lti=False)
(the recursion and the transposing stage body, untouched) bit for bit.

A converged solve hides a wrong K, because the interior-point iteration corrects itself: the cases that count stop
after one and after two iterations, where z is one or two Newton steps with that K.  The uncapped solve is compared
as well (z, kkt, iters, status).

Horizons at the tile and segment edges (nu = 2, 16 columns per tile, 8 stages per segment): 8 one full tile |
9 two columns in the second, the segment's own, tile | 16, 17 the same one tile on | 24 three full tiles, run by
the four-tile instantiation (mpc3_tiles) | 25 | 30 the workload's | 32 no padding column.  Neighbours 0, 1, 2.
The population is time-invariant with dense perturbed A and B (as test_v3_lti_gpu.py's "dense"), so that no
structural zero of the table can hide a wrong slot or component.

N = 9 and 16 run the two-tile instantiation, which keeps the transposing stage body (tf_on): with the in-place body
[16-1-2] and [16-1-None] failed (56 of 80 agents, max |dz| 0.12; the first iteration equal), and with the
transposing body on the new images [16-2-*] did instead; the cause is not found."""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZONS = [8, 9, 16, 17, 24, 25, 30, 32]
NBS = [0, 1, 2]
CAPS = [1, 2, None]   # max_iter: one Newton step, two, the solver's default
AGENTS = 80
EPS, SEED = 1e-2, 20240
OUT = ("z", "kkt", "iters", "status")


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
def test_fragments_in_place_bit_equal_to_recursion(gpu_ctx, N, nb, cap):
    from cmpc import _lib as L
    from cmpc.rounds import is_lti

    sc = scenario(N, nb)
    assert is_lti(sc.A, sc.B) and np.count_nonzero(sc.A[:, 0]) == sc.A[:, 0].size
    T, t = one_round(gpu_ctx, sc, True, cap)
    G, g = one_round(gpu_ctx, sc, False, cap)
    assert T.opts.flags & L.CMPC_FLAG_LTI and not G.opts.flags & L.CMPC_FLAG_LTI
    assert np.isfinite(g["z"]).all()
    if cap is not None:
        # the cap binds: z is the iterate after exactly cap Newton steps
        assert (g["iters"] == cap).all(), g["iters"]
    for a in OUT:
        assert np.array_equal(t[a], g[a]), (a, int((t[a] != g[a]).sum()))
