"""The v3 kernel's pivot verdict (mpc_ipm3.hip, pivot_acc_on; DESIGN.md §3, "third census pass"): each of the
factorisation's pivot tests `!(d_jj > 0)` is taken at the pivot and or-ed into one running scalar lane mask, and the
breakdown exit is a scalar branch on that mask.  No floating-point operation changes, so nothing may change by a bit,
on the healthy path and on the breakdown path.

Healthy path: two consecutive rounds of DIRounds(fused=True), the structured DS / TI instantiations with the rows
built in the launch, against DIRounds(fused=False), the dense instantiation behind di_build_kernel, with and without
the time-invariance promise, stopped after one and after two iterations and uncapped.  z, kkt, iters, status and the
exchanged x0, u_prev, traj_all are compared as 64-bit patterns.  Horizons (nu = 2, 16 columns per tile): 8 one full
tile | 9, 16 the two-tile instantiation at both ends | 17 the first three-tile horizon | 25 four tiles with padding |
30 the workload's.  Neighbours 0 and 2.  Five agents: not a multiple of the four per CU.

Breakdown path, at N = 30 and N = 9 (nb = 2), by the input weight R of the first round's problems:
  first     R = -1e6 I: the first pivot of the first block is negative;
  later     R = -eps I, eps such that the columns of the first 16 x 16 block, whose stages carry more Gamma'W Gamma
            curvature, keep positive pivots and the first non-positive pivot falls in a later block (checked on a
            numpy restatement of the first iteration's Newton matrix, `_first_K`): eps = 5, column 19 at N = 30 and
            column 16 at N = 9 (both the second block);
  last      (N = 30) eps = 1: column 58, the fourth block, so the verdict hangs on one of the last tests or-ed in;
  nan       R[0][0] = NaN: the first pivot is NaN (not `> 0`, so a breakdown; the restatement stops it with the
            same status in the same iteration).
Each case is chosen on the CPU alone and asserted here, so the test cannot pass by not breaking down: the C
restatement (oracle.cmpc_oracle.solve_batch) must end every agent at CMPC_UNSOLVED in its first iteration.  Without
CMPC_FLAG_RESCUE the fused round must match build-then-solve bit for bit in every output, and the restatement in
status and iters; with it (the exit then writes the iterate's image and the workspace stamp for the Riccati
continuation) the final z, status and iters of the two must be bit-equal."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZONS = [8, 9, 16, 17, 25, 30]
NBS = [0, 2]
CAPS = [1, 2, None]   # max_iter: one Newton step, two, the solver's default
AGENTS = 5
ROUNDS = 2
OUT = ("z", "kkt", "iters", "status", "x0", "u_prev", "traj_all")
UNSOLVED = -10        # CMPC_UNSOLVED
T0_FLOOR_COND = 0.1   # the condensed method's floor of the starting slacks (internal.h kT0FloorCond)
EPS = {"later": 5.0, "last": 1.0}   # R = -eps I
BLOCK = {(30, "later"): 1, (30, "last"): 3, (9, "later"): 1}   # the 16-column block of the first non-positive pivot
CASES = [(30, "first"), (30, "later"), (30, "last"), (30, "nan"), (9, "first"), (9, "later"), (9, "nan")]


def _scenario(N, nb, kind=None):
    from cmpc import scenarios as S

    sc = S.make_di(AGENTS, N, nb, 2)
    if kind is not None:
        nu = sc.shared["nu"]
        R = np.zeros((nu, nu)) if kind == "nan" else -(1e6 if kind == "first" else EPS[kind]) * np.eye(nu)
        if kind == "nan":
            R[0, 0] = np.nan
        sc.shared["R"] = R
    return sc


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _read(R, names):
    return {a: getattr(R, a).detach().cpu().numpy().copy() for a in names}


def _assert_bit_equal(f, u, names, what):
    for a in names:
        fb, ub = _bits(f[a]), _bits(u[a])
        assert fb.shape == ub.shape and np.array_equal(fb, ub), (what, a, int((fb != ub).sum()))


def _rounds_equal(gpu_ctx, sc, lti, cap):
    """ROUNDS consecutive rounds, fused against build-then-solve."""
    import torch
    from cmpc.rounds import DIRounds

    F = DIRounds(sc, ctx=gpu_ctx, fused=True, lti=lti, max_iter=cap)
    U = DIRounds(sc, ctx=gpu_ctx, fused=False, lti=lti, max_iter=cap)
    for rnd in range(ROUNDS):
        F.step()
        U.step()
        torch.cuda.synchronize()
        f, u = _read(F, OUT), _read(U, OUT)
        assert np.isfinite(u["z"]).all(), (lti, cap, rnd)
        if cap is not None:
            assert (u["iters"] == cap).all(), (lti, cap, rnd, u["iters"])   # the cap binds
        _assert_bit_equal(f, u, OUT, (lti, cap, rnd))


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("N", HORIZONS)
def test_fused_rounds_bit_equal_to_build_then_solve(gpu_ctx, N, nb):
    sc = _scenario(N, nb)
    for lti in (True, False):
        for cap in CAPS:
            _rounds_equal(gpu_ctx, sc, lti, cap)


def _first_K(P, a):
    """The condensed Newton matrix of agent `a`'s first iteration, as the C restatement forms it (cmpc_oracle.c,
    "Newton matrix"): the start U = 0, sigma = 0, lambda = 1, t = max(w - g, floor), theta = lambda / t."""
    nx, nu, N, ns, mc = (int(P[k]) for k in ("nx", "nu", "N", "ns", "mc"))
    n = N * nu
    A, B, C, h = P["A"][a], P["B"][a], P["C"][a], P["h"][a]
    slack, sign = np.asarray(P["row_slack"]), np.asarray(P["row_sign"], float)
    Qs = np.asarray(P["Qs"], float).reshape(-1)
    Gam = np.zeros((N + 1, nx, n))
    X = np.zeros((N + 1, nx))
    X[0] = P["x0"][a]
    for k in range(N):
        Gam[k + 1] = A[k] @ Gam[k]
        Gam[k + 1][:, k * nu:(k + 1) * nu] += B[k]
        X[k + 1] = A[k] @ X[k]
    g = np.einsum("krs,ks->kr", C, X[1:])
    th = np.where(np.isfinite(h), 1.0 / np.maximum(h - g, T0_FLOOR_COND), 0.0)
    K = np.zeros((n, n))
    for k in range(N):
        W = 2.0 * np.asarray(P["Q"], float)
        for r in range(mc):
            j = slack[r]
            if j < 0:
                W = W + th[k, r] * np.outer(C[k, r], C[k, r])
                continue
            inv = 1.0 / (2.0 * Qs[j] + th[k, slack == j].sum())
            W = W + 2.0 * Qs[j] * th[k, r] * inv * np.outer(C[k, r], C[k, r])
            for r2 in range(r + 1, mc):
                if slack[r2] == j:
                    d = sign[r] * C[k, r] - sign[r2] * C[k, r2]
                    W = W + th[k, r] * th[k, r2] * inv * np.outer(d, d)
        K += Gam[k + 1].T @ W @ Gam[k + 1]
    R, dR = np.asarray(P["R"], float), np.asarray(P["dR"], float)
    ub, lb = np.asarray(P["u_ub"], float), np.asarray(P["u_lb"], float)
    thu = np.where(np.isfinite(ub), 1.0 / np.maximum(ub, T0_FLOOR_COND), 0.0) + \
        np.where(np.isfinite(lb), 1.0 / np.maximum(-lb, T0_FLOOR_COND), 0.0)
    for k in range(N):
        s = slice(k * nu, (k + 1) * nu)
        K[s, s] += 2.0 * R + 2.0 * dR * (2.0 if k + 1 < N else 1.0) + np.diag(thu)
        if k > 0:
            p = slice((k - 1) * nu, k * nu)
            K[s, p] += -2.0 * dR
            K[p, s] += -2.0 * dR.T
    return K


def _pivots(K):
    """The Cholesky pivots d_jj of K up to and including the first that is not > 0 (the solver's test)."""
    n = K.shape[0]
    L = np.zeros((n, n))
    d = []
    for j in range(n):
        djj = K[j, j] - L[j, :j] @ L[j, :j]
        d.append(djj)
        if not djj > 0.0:
            break
        L[j, j] = np.sqrt(djj)
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return np.array(d)


@functools.lru_cache(maxsize=None)
def _breakdown_case(N, kind):
    """The first round's problems of a breakdown case, and the C restatement's status / iters (read-only)."""
    from oracle import cmpc_oracle as CO
    from oracle import synth

    sc = _scenario(N, 2, kind)
    P = synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj,
                         np.arange(AGENTS))
    _, _, it, st = CO.solve_batch(P)
    it.setflags(write=False)
    st.setflags(write=False)
    return P, it, st


def _assert_breaks_down_as_intended(N, kind):
    P, it, st = _breakdown_case(N, kind)
    assert (st == UNSOLVED).all() and (it == 1).all(), (N, kind, st, it)
    for a in range(AGENTS):
        K = _first_K(P, a)
        d = _pivots(K)
        scale = np.abs(K[np.isfinite(K)]).max()
        if kind == "first":
            assert len(d) == 1 and d[0] < -1e-6 * scale, (N, a, d)
        elif kind == "nan":
            assert len(d) == 1 and np.isnan(d[0]), (N, a, d)
        else:   # every earlier pivot positive, the failing one in the intended later block; both clear of rounding
            assert (len(d) - 1) // 16 == BLOCK[N, kind] and d[:-1].min() > 1e-6 * scale and d[-1] < -1e-6 * scale, \
                (N, kind, a, len(d), d)


@pytest.mark.parametrize("N,kind", CASES)
def test_breakdown_without_rescue(gpu_ctx, N, kind):
    import torch
    from cmpc.rounds import DIRounds

    _assert_breaks_down_as_intended(N, kind)
    _, itc, stc = _breakdown_case(N, kind)
    sc = _scenario(N, 2, kind)
    for lti in (True, False):
        F = DIRounds(sc, ctx=gpu_ctx, fused=True, lti=lti)
        U = DIRounds(sc, ctx=gpu_ctx, fused=False, lti=lti)
        F.step()
        U.step()
        torch.cuda.synchronize()
        f, u = _read(F, OUT), _read(U, OUT)
        _assert_bit_equal(f, u, OUT, (N, kind, lti))
        assert np.array_equal(f["status"], stc) and np.array_equal(f["iters"], itc), \
            (N, kind, lti, f["status"], f["iters"], stc, itc)


@pytest.mark.parametrize("N,kind", CASES)
def test_breakdown_with_rescue(gpu_ctx, N, kind):
    import torch
    from cmpc import _lib as L
    from cmpc.rounds import DIRounds

    _assert_breaks_down_as_intended(N, kind)
    sc = _scenario(N, 2, kind)
    for lti in (True, False):
        F = DIRounds(sc, ctx=gpu_ctx, fused=True, lti=lti)
        U = DIRounds(sc, ctx=gpu_ctx, fused=False, lti=lti)
        for R in (F, U):
            R.opts.flags |= L.CMPC_FLAG_RESCUE
        F.step()
        U.step()
        torch.cuda.synchronize()
        names = ("z", "status", "iters")
        _assert_bit_equal(_read(F, names), _read(U, names), names, (N, kind, lti))
