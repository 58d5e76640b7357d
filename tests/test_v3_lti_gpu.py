"""CMPC_FLAG_LTI on the fused double-integrator round (mpc_ipm3.hip, the TI instantiation): the K build reads
the columns of the condensed dynamics from a table built once per solve instead of carrying them through
A_k Gamma_k in every iteration.  The table holds the same fmas on the same operands in the same order, so a
round with the flag is bit for bit the round without it: every output and every piece of round state is
compared with np.array_equal after every round, on the shapes at which the tile and segment logic changes.

Two time-invariant populations: make_di as it is, and make_di with every agent's A, B replaced by the
integrator's plus a seeded dense perturbation (so the table path cannot lean on the integrator's zeros).  The
perturbation's size EPS was chosen on the CPU: with it oracle.cmpc_oracle.solve_batch ends at status 1 for every
agent of every shape below in each of the three rounds (the rounds advanced on the host as the device does);
3e-2 already leaves agents at other statuses.  One time-varying population: the flag must not be set by default,
and the results must be those of the unfused path.

N = 24 (n = 48) and the four-tile instantiation: three tiles with fewer than four padding columns gave wrong
Newton directions whatever the flag (status -10 / -2 on the dense population here, which the C oracle solves in
16 iterations), so such horizons run the four-tile instantiation (mpc3_tiles, mpc_ipm3.hip)."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("z", "kkt", "iters", "status", "x0", "u_prev", "traj_local", "traj_all")
# (N, nb): one tile, unsegmented recursions | first two-tile, segmented shape | n = 48, three full tiles |
# n = 50, four tiles, padded | the workload's shape | n = 64, no padding lane
SHAPES = [(8, 2), (9, 1), (24, 2), (25, 0), (30, 2), (32, 2)]
AGENTS, ROUNDS = 8, 3
EPS, SEED = 1e-2, 20240


def perturbed(sc, eps=EPS, seed=SEED):
    """sc with every agent's (time-invariant) A, B replaced by Ad, Bd plus eps x a seeded dense normal matrix."""
    rng = np.random.default_rng(seed)
    n, N, nx, nu = sc.n_agents, sc.N, sc.A.shape[2], sc.B.shape[3]
    dA = eps * rng.standard_normal((n, 1, nx, nx))
    dB = eps * rng.standard_normal((n, 1, nx, nu))
    A = np.ascontiguousarray(np.broadcast_to(sc.A[:, :1] + dA, (n, N, nx, nx)))
    B = np.ascontiguousarray(np.broadcast_to(sc.B[:, :1] + dB, (n, N, nx, nu)))
    return dataclasses.replace(sc, A=A, B=B)


def scenario(N, nb, pop):
    from cmpc import scenarios as S

    sc = S.make_di(AGENTS, N, nb, 2)
    return perturbed(sc) if pop == "dense" else sc


def state(R):
    import torch

    torch.cuda.synchronize()
    return {a: getattr(R, a).detach().cpu().numpy().copy() for a in STATE}


@pytest.mark.parametrize("pop", ["integrator", "dense"])
@pytest.mark.parametrize("N,nb", SHAPES)
def test_lti_rounds_bit_equal_to_recursion(gpu_ctx, N, nb, pop):
    from cmpc import _lib as L
    from cmpc.rounds import DIRounds, is_lti

    sc = scenario(N, nb, pop)
    assert is_lti(sc.A, sc.B)
    T = DIRounds(sc, ctx=gpu_ctx, lti=True)
    G = DIRounds(sc, ctx=gpu_ctx, lti=False)
    assert T.opts.flags & L.CMPC_FLAG_LTI and not G.opts.flags & L.CMPC_FLAG_LTI
    assert DIRounds(sc, ctx=gpu_ctx).opts.flags & L.CMPC_FLAG_LTI   # the default finds it
    for rnd in range(ROUNDS):
        T.step()
        G.step()
        t, g = state(T), state(G)
        for a in STATE:
            assert np.array_equal(t[a], g[a]), (rnd, a)
        assert (t["status"] == 1).all() and (g["status"] == 1).all(), (rnd, t["status"], g["status"])


def test_time_varying_population_keeps_the_recursion(gpu_ctx):
    """One stage of one agent's A off by 1e-2: the default must not promise LTI, and the fused round (torch-driven
    and through the C handle, whose create runs the same test on its host arrays) must give the unfused path's
    bits.  Reading stage 0 only would move z by far more than rounding."""
    from cmpc import _lib as L
    from cmpc import scenarios as S
    from cmpc.rounds import DIRounds, DIRoundsHandle, is_lti

    sc = S.make_di(AGENTS, 30, 2, 2)
    A = sc.A.copy()
    A[3, 17, 0, 2] += 1e-2
    sc = dataclasses.replace(sc, A=A)
    assert not is_lti(sc.A, sc.B)
    F = DIRounds(sc, ctx=gpu_ctx)
    U = DIRounds(sc, ctx=gpu_ctx, fused=False)
    assert not F.opts.flags & L.CMPC_FLAG_LTI
    F.step()
    U.step()
    f, u = state(F), state(U)
    for a in STATE:
        assert np.array_equal(f[a], u[a]), a
    H = DIRoundsHandle(sc, ctx=gpu_ctx)
    assert H.step(1) == 1
    r = H.read()
    for a in ("z", "kkt", "iters", "status", "x0", "u_prev"):
        assert np.array_equal(r[a], f[a]) and np.array_equal(r[a], u[a]), a
    H.close()
    # the stage-0 model's solution is a different one: the comparison above can tell
    W = DIRounds(sc, ctx=gpu_ctx, lti=True)
    W.step()
    assert np.abs(state(W)["z"] - f["z"]).max() > 1e-6
