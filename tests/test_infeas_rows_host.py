"""The numpy statement of the combined-row infeasibility certificate (cmpc.infeas.certify_rows, the rule of
csrc/mpc_infeas_rows.hip) on the CPU: agents whose hard rows are each reachable alone but contradict each other
(which the single-row rule, cmpc.infeas.certify, does not catch) are certified within the iteration cap, the ray
verifies on the reference-form matrices, an independent dense formulation of the iteration certifies at the same
iteration, and the cases that must get no certificate get none."""
import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import infeas, structure
from test_infeas_gpu import BATCH, SHAPES, problem
from test_infeas_host import dense_reach

GAP = 0.3
# one hard row type (r), a contradiction planted at stage k; too long for the kernel's LDS copy of the stage data:
LONG = [((9, 2, 125, 3, 7), [0, 1, 2, -1, 0, 1, 2], 3, 100),    # the reference's horizon at nx = 9
        ((9, 2, 125, 3, 6), [-1, 0, 1, 1, 2, 2], 0, 100)]       # ... with the LPV car's row pattern


def dense_reach_max(p, a, k, r):
    """max of C[k, r] x_k over the input box: minus the min of the negated row."""
    q = dict(p, C=-p["C"])
    return -dense_reach(q, a, k, r)


def plant_pair(p, a, k, r1, r2, gap=GAP):
    """Row r2 of stage k becomes the negated row r1; h1 = the midpoint of r1's reachable range and the second
    bound -(h1 + gap): c'x_k <= h1 and c'x_k >= h1 + gap."""
    p["C"][a, k - 1, r2] = -p["C"][a, k - 1, r1]
    h1 = 0.5 * (dense_reach(p, a, k, r1) + dense_reach_max(p, a, k, r1))
    p["h"][a, k - 1, r1] = h1
    p["h"][a, k - 1, r2] = -(h1 + gap)


def planted_rows(i):
    """Shape i of tests/test_infeas_gpu.py (its seeds) with one contradictory pair of hard rows per agent, at
    stage 1, N, the middle, 2, N - 1 and N // 3 + 1; returns (problem, stages)."""
    shape, slack = SHAPES[i]
    nx, nu, N, ns, mc = shape
    p = problem(shape, slack, 10 + i)
    hard = [r for r in range(mc) if slack[r] < 0]
    ks = [1, N, (N + 1) // 2, 2, N - 1, N // 3 + 1]
    for a, k in enumerate(ks):
        plant_pair(p, a, k, hard[0], hard[-1])
    return p, ks


def plant_consecutive(p, a, k, r, gap=GAP):
    """One hard row type, two consecutive stages that contradict each other through the dynamics.  With
    c = C[k, r] and c2 = -A_k^-T c the row c2'x_{k+1} <= h2 reads -c'x_k + c2'B_k u_k <= h2, so with c'x_k <= h1
    (h1 = the midpoint of the row's reachable range) it needs -h1 + min_u c2'B_k u_k <= h2: h2 = that bound - gap."""
    c = p["C"][a, k - 1, r]
    c2 = -np.linalg.solve(p["A"][a, k].T, c)
    p["C"][a, k, r] = c2
    h1 = 0.5 * (dense_reach(p, a, k, r) + dense_reach_max(p, a, k, r))
    coef = c2 @ p["B"][a, k]
    umin = np.where(coef > 0, coef * p["u_lb"], coef * p["u_ub"]).sum()
    p["h"][a, k - 1, r] = h1
    p["h"][a, k, r] = -h1 + umin - gap


def long_problem(which=0, seed=20):
    """One agent at a long horizon with a single hard row type (plant_consecutive at stage k).  Every other hard
    row has an infinite bound (inactive) but for five at h = 50."""
    shape, slack, r, k = LONG[which]
    nx, nu, N, ns, mc = shape
    rng = np.random.default_rng(seed)
    p = dict(nx=nx, nu=nu, N=N, ns=ns, mc=mc, Q=np.eye(nx), R=np.eye(nu), dR=np.eye(nu), Qs=np.ones(ns),
             u_ub=np.array([1.0, 2.0]), u_lb=np.array([-0.5, -1.5]), row_slack=np.array(slack, np.int32),
             row_sign=np.ones(mc, np.int32),
             A=0.98 * np.eye(nx) + 0.05 * rng.standard_normal((1, N, nx, nx)) / np.sqrt(nx),
             B=0.5 * rng.standard_normal((1, N, nx, nu)), x0=rng.standard_normal((1, nx)),
             u_prev=np.zeros((1, nu)), qlin=rng.standard_normal((1, N + 1, nx)),
             C=rng.standard_normal((1, N, mc, nx)), h=np.full((1, N, mc), 50.0))
    p["h"][0, :, r] = np.inf
    p["h"][0, [4, 40, 80, 110, 124], r] = 50.0
    plant_consecutive(p, 0, k, r)
    return p


_CACHE = {}


def reference(i):
    """(problem, stages, certify(p), certify_rows(p)) of shape i (from len(SHAPES): the long horizons), computed
    once."""
    if i not in _CACHE:
        p, ks = planted_rows(i) if i < len(SHAPES) else (long_problem(i - len(SHAPES)), [LONG[i - len(SHAPES)][3]])
        _CACHE[i] = (p, ks, infeas.certify(p), infeas.certify_rows(p))
    return _CACHE[i]


def check_rows_ray(p, a, y, d=None, S=None):
    _, _, G, h, Aeq, beq = structure.reference_form(p, a)
    res, gap = infeas.verify(G, h, Aeq, beq, y)
    assert res <= 1e-12 * np.abs(y).max(), (a, res)
    assert gap < 0, (a, gap)
    assert (y[:h.size] >= 0).all()
    if d is not None:
        assert abs(gap + d) <= 1e-12 * S, (a, gap, d, S)
    return res, gap


def dense_rows(p, a, max_iter=infeas.CERT_ROWS_MAX_ITER, check_every=infeas.CERT_ROWS_CHECK_EVERY):
    """An independent formulation of the rule for agent a: the condensed matrix of the hard rows built explicitly
    (as dense_reach), v = max(M u + c0 - h, 0), gradient M'v.  Returns (certified, iters, normalised w over the
    rows of H in stage order, d / S)."""
    nx, nu, N, mc = p["nx"], p["nu"], p["N"], p["mc"]
    lb, ub = np.tile(p["u_lb"], N), np.tile(p["u_ub"], N)
    rows, c0, hh = [], [], []
    Phi, Gam = np.eye(nx), np.zeros((nx, N * nu))
    for j in range(N):
        Gam = p["A"][a, j] @ Gam
        Gam[:, j * nu:(j + 1) * nu] = p["B"][a, j]
        Phi = p["A"][a, j] @ Phi
        for r in range(mc):
            if p["row_slack"][r] < 0 and np.isfinite(p["h"][a, j, r]):
                rows.append(p["C"][a, j, r] @ Gam)
                c0.append(p["C"][a, j, r] @ Phi @ p["x0"][a])
                hh.append(p["h"][a, j, r])
    M, c0, hh = np.array(rows), np.array(c0), np.array(hh)
    step = 1.0 / (M ** 2).sum()
    u = np.clip(np.zeros(N * nu), lb, ub)
    y, t = u.copy(), 1.0
    for it in range(1, max_iter + 1):
        v = np.maximum(M @ y + c0 - hh, 0.0)
        un = np.clip(y - (M.T @ v) * step, lb, ub)
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        y = un + ((t - 1.0) / tn) * (un - u)
        u, t = un, tn
        if it % check_every and it != max_iter:
            continue
        w = np.maximum(M @ u + c0 - hh, 0.0)
        if w.max() == 0.0:
            return False, it, w, 0.0
        w = w / w.max()
        g = w @ M
        bnd = np.where(g > 0, lb, ub)
        reach = w @ c0 + (g * bnd)[g != 0].sum()
        # (S with the aggregate's own x0 term: |P_0s x0_s| summed per state, so rebuilt from the stage recursion)
        d = reach - w @ hh
        if d > 0 and d > infeas.CERT_TOL * (np.abs(w * hh).sum() + np.abs(g * bnd).sum() + abs(w @ c0)):
            return True, it, w, d
    return False, max_iter, w, d


ALL = range(len(SHAPES) + len(LONG))


def test_constants():
    assert L.CMPC_FLAG_CERTIFY_ROWS == 8192 and infeas.CERT_ROWS_MAX_ITER == 512
    assert infeas.CERT_ROWS_CHECK_EVERY == 8


@pytest.mark.parametrize("i", ALL)
def test_planted_agents_are_beyond_the_single_row_rule_and_are_certified(i):
    p, ks, single, ref = reference(i)
    B = p["A"].shape[0]
    assert (single["row"] == -1).all() and (single["status"] == 0).all(), single["row"]
    print(f"shape {i}: iters {ref['iters']} nrows {ref['nrows']} margin {ref['margin']}")
    assert (ref["status"] == L.CMPC_PRIMAL_INFEASIBLE).all(), ref["status"]
    assert (ref["iters"] <= infeas.CERT_ROWS_MAX_ITER).all() and (ref["nrows"] >= 2).all()
    # no check sat on the threshold: a seed within 1e-6 relative of it would make iters a matter of rounding
    assert (ref["margin"] > infeas.CERT_TOL * (1 + 1e-6)).all()


@pytest.mark.parametrize("i", ALL)
def test_ray_verifies_on_the_reference_form(i):
    p, ks, _, ref = reference(i)
    for a in range(p["A"].shape[0]):
        d = ref["margin"][a] * ref["scale"][a]
        res, gap = check_rows_ray(p, a, ref["ray"][a], d, ref["scale"][a])
        print(f"shape {i} agent {a}: residual {res:.2e} gap {gap:.6f} d {d:.6f}")


@pytest.mark.parametrize("i", ALL)
def test_dense_formulation_certifies_at_the_same_iteration(i):
    p, ks, _, ref = reference(i)
    hard = np.asarray(p["row_slack"]) < 0
    dev = 0.0
    for a in range(p["A"].shape[0]):
        ok, it, w, d = dense_rows(p, a)
        Hm = hard[None, :] & np.isfinite(p["h"][a])
        wr = ref["ray"][a][:p["N"] * p["mc"]].reshape(p["N"], p["mc"])[Hm]
        assert ok and it == ref["iters"][a], (a, it, ref["iters"][a])
        dev = max(dev, np.abs(w - wr).max(), abs(d - ref["margin"][a] * ref["scale"][a]) / ref["scale"][a])
    print(f"shape {i}: stage recursions against the condensed matrix {dev:.2e}")
    assert dev <= 1e-10, dev


def test_no_certificate():
    p0, ks, _, ref = reference(0)
    ce = infeas.CERT_ROWS_CHECK_EVERY

    def one(p, **kw):
        return infeas.certify_rows(p, **kw)

    # a feasible agent stops at a check with margin 0
    p = problem(*SHAPES[0], 10)
    r = one(p)
    assert (r["status"] == 0).all() and (r["margin"] == 0.0).all() and np.isnan(r["ray"]).all()
    assert (r["iters"] <= ce * 4).all() and (r["iters"] % ce == 0).all() and (r["nrows"] == 0).all()
    # an impossible bound on soft rows only
    p = problem(*SHAPES[0], 10)
    p["h"][:, :, 1] = -1e3
    r = one(p)
    assert (r["status"] == 0).all() and (r["margin"] == 0.0).all()
    # an infinite bound on an input the aggregate touches
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p0.items()}
    p["u_ub"] = np.array([np.inf, np.inf])
    p["u_lb"] = np.array([-np.inf, -np.inf])
    r = one(p, max_iter=64)
    assert (r["status"] == 0).all() and np.isnan(r["ray"]).all()
    # NaN in x0 or A
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p0.items()}
    p["x0"][0, 1] = np.nan
    p["A"][1, 1, 0, 0] = np.nan
    r = one(p)
    assert list(r["status"][:2]) == [0, 0] and np.isnan(r["margin"][:2]).all() and np.isnan(r["ray"][:2]).all()
    assert r["iters"][0] == ce and r["iters"][1] == 0
    assert (r["status"][2:] == -3).all()
    assert np.array_equal(r["ray"][2:], ref["ray"][2:]) and np.array_equal(r["iters"][2:], ref["iters"][2:])
    # an empty box; no hard rows
    p = dict(p0, u_lb=np.array([2.0, -1.0]))
    r = one(p)
    assert (r["status"] == 0).all() and np.isnan(r["margin"]).all() and (r["iters"] == 0).all()
    p = dict(p0, row_slack=np.zeros(3, np.int32))
    r = one(p)
    assert (r["status"] == 0).all() and np.isnan(r["margin"]).all() and (r["iters"] == 0).all()
    # status 1, 2 and -3 are skipped with nothing written
    st = np.array([1, 2, -3, -2, -10, 0], np.int32)
    r = one(p0, status=st)
    assert list(r["status"]) == [1, 2, -3, -3, -3, -3]
    assert np.isnan(r["ray"][:3]).all() and np.isnan(r["margin"][:3]).all() and (r["iters"][:3] == 0).all()
    assert np.array_equal(r["ray"][3:], ref["ray"][3:])
    # ... as the single-row rule's own -3 is: an agent with an unreachable row as well keeps that certificate
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p0.items()}
    p["h"][0, 2, 0] = dense_reach(p, 0, 3, 0) - GAP
    single = infeas.certify(p)
    r = one(p, status=single["status"])
    assert single["status"][0] == -3 and np.isnan(r["ray"][0]).all() and r["iters"][0] == 0
    assert np.array_equal(r["ray"][1:], ref["ray"][1:])
