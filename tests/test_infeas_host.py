"""The numpy statement of the infeasibility certificate (cmpc.infeas.certify: single-row reachability, the rule
of csrc/mpc_infeas.hip) and the ray check (cmpc.infeas.verify), on the CPU: the reach against an independent
dense computation (the condensed dynamics built explicitly), the Farkas ray against the reference-form
matrices of cmpc.structure.reference_form, and the cases that must get no certificate."""
import numpy as np

from cmpc import _lib as L
from cmpc import infeas, structure

NX, NU, N, NS, MC = 3, 2, 5, 1, 3


def base_problem(seed=0, batch=1):
    """Seeded random agents: rows 0 and 2 hard, row 1 soft; input 1 has no upper bound.  Row 0 has positive
    coefficients and B a positive second column, so its minimising bound on input 1 is the finite lower one; row
    2 is its negative, so its minimising bound there is the infinite one.  h = 50 everywhere: feasible."""
    rng = np.random.default_rng(seed)
    A = np.eye(NX) + 0.1 * rng.standard_normal((batch, N, NX, NX))
    B = 0.5 * rng.standard_normal((batch, N, NX, NU))
    B[..., 1] = 0.2 + np.abs(B[..., 1])
    C = rng.standard_normal((batch, N, MC, NX))
    C[:, :, 0] = 0.2 + np.abs(C[:, :, 0])
    C[:, :, 2] = -C[:, :, 0]
    return dict(nx=NX, nu=NU, N=N, ns=NS, mc=MC, Q=np.eye(NX), R=np.eye(NU), dR=np.eye(NU), Qs=np.ones(NS),
                u_ub=np.array([1.0, np.inf]), u_lb=np.array([-1.0, -2.0]), row_slack=np.array([-1, 0, -1], np.int32),
                row_sign=np.array([1, 1, 1], np.int32), A=A, B=B, x0=rng.standard_normal((batch, NX)),
                u_prev=np.zeros((batch, NU)), qlin=rng.standard_normal((batch, N + 1, NX)), C=C,
                h=np.full((batch, N, MC), 50.0))


def dense_reach(p, a, k, r):
    """min of C[k, r] x_k over the input box, from x_k = Phi x0 + Gamma u with Gamma built explicitly."""
    nx, nu = p["nx"], p["nu"]
    Phi, Gam = np.eye(nx), np.zeros((nx, k * nu))
    for j in range(k):
        Gam = p["A"][a, j] @ Gam
        Gam[:, j * nu:(j + 1) * nu] = p["B"][a, j]
        Phi = p["A"][a, j] @ Phi
    c = p["C"][a, k - 1, r]
    coef = c @ Gam
    lo, hi = np.tile(p["u_lb"], k), np.tile(p["u_ub"], k)
    with np.errstate(invalid="ignore"):
        terms = np.where(coef > 0, coef * lo, np.where(coef < 0, coef * hi, 0.0))
    return float(c @ Phi @ p["x0"][a] + terms.sum())


def check_ray(p, a, y, gap):
    _, _, G, h, Aeq, beq = structure.reference_form(p, a)
    res, got = infeas.verify(G, h, Aeq, beq, y)
    assert res <= 1e-12 * np.abs(y).max(), res
    assert abs(got - gap) <= 1e-12, (got, gap)
    assert (y[:h.size] >= 0).all()


def test_flag_value():
    assert L.CMPC_FLAG_CERTIFY == 4096 and L.CMPC_PRIMAL_INFEASIBLE == -3 and infeas.CERT_TOL == 1e-9


def test_unreachable_row_is_certified_with_a_farkas_ray():
    for k in (1, 3, N):
        p = base_problem()
        reach = dense_reach(p, 0, k, 0)
        assert np.isfinite(reach)
        p["h"][0, k - 1, 0] = reach - 0.3
        c = infeas.certify(p)
        assert c["row"][0] == (k - 1) * MC and c["status"][0] == L.CMPC_PRIMAL_INFEASIBLE
        assert c["margin"][0] > infeas.CERT_TOL
        check_ray(p, 0, c["ray"][0], -0.3)


def test_winner_is_the_largest_ratio_and_ties_go_to_the_first_row():
    p = base_problem()
    for k, gap in ((2, 0.3), (4, 5.0)):
        p["h"][0, k - 1, 0] = dense_reach(p, 0, k, 0) - gap
    c = infeas.certify(p)
    assert c["row"][0] == 3 * MC
    check_ray(p, 0, c["ray"][0], -5.0)
    # two identical rows (r = 0 and a hard copy of it at r = 1) tie exactly: the smaller r
    q = base_problem()
    q["row_slack"] = np.array([-1, -1, -1], np.int32)
    q["C"][:, :, 1] = q["C"][:, :, 0]
    h3 = dense_reach(q, 0, 3, 0) - 1.0
    q["h"][0, 2, 0] = q["h"][0, 2, 1] = h3
    assert infeas.certify(q)["row"][0] == 2 * MC


def test_no_certificate():
    def none(p, status=None):
        c = infeas.certify(p, status)
        assert c["row"][0] == -1 and np.isnan(c["ray"][0]).all()
        return c

    p = base_problem()
    c = none(p)                                   # h = 50 everywhere: feasible, a negative margin
    assert c["margin"][0] < 0 and c["status"][0] == 0
    p["h"][0, :, 1] = -1e3                        # an impossible bound on the soft row only: its slack takes it
    none(p)
    p["h"][0, :, 2] = -1e6                        # row 2's minimising bound on input 1 is the infinite one
    assert none(p)["margin"][0] < 0               # (row 0 is still the only candidate)
    p = base_problem()
    p["C"][:, :, 0] = -p["C"][:, :, 0]            # ... and with both hard rows disqualified: no candidate at all
    assert np.isnan(none(p)["margin"][0])
    for key in ("x0", "A"):                       # NaN data under a planted unreachable row
        p = base_problem()
        p["h"][0, 2, 0] = dense_reach(p, 0, 3, 0) - 0.3
        assert infeas.certify(p)["row"][0] == 2 * MC
        p[key] = p[key].copy()
        p[key][(0,) * p[key].ndim] = np.nan
        assert np.isnan(none(p)["margin"][0])
    p = base_problem()                            # an empty input box: no certificate attempted
    p["h"][0, 2, 0] = dense_reach(p, 0, 3, 0) - 0.3
    p["u_lb"] = np.array([2.0, -2.0])
    assert np.isnan(none(p)["margin"][0])


def test_status_selects_the_agents_and_infinite_bounds_are_inactive():
    p = base_problem(batch=3)
    for a in range(3):
        p["h"][a, 1, 0] = dense_reach(p, a, 2, 0) - 0.3
    c = infeas.certify(p, np.array([1, -2, 2], np.int32))
    assert list(c["status"]) == [1, -3, 2] and list(c["row"]) == [-1, MC, -1]
    assert np.isnan(c["ray"][[0, 2]]).all() and np.isnan(c["margin"][[0, 2]]).all()
    # a row with an infinite bound is no candidate, and verify counts its entry of y as 0
    p["h"][1, 1, 0] = np.inf
    assert infeas.certify(p)["row"][1] == -1
    _, _, G, h, Aeq, beq = structure.reference_form(p, 1)
    y = np.zeros(G.shape[0] + Aeq.shape[0])
    y[MC] = 7.0
    assert infeas.verify(G, h, Aeq, beq, y) == (0.0, 0.0)
