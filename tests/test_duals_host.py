"""CPU checks of the dual solution's definition (cmpc.duals.recover, the numpy statement of
csrc/mpc_dual.hip): on every captured reference QP the costate recursion reproduces the certified
equality multipliers from the certified z and inequality multipliers, the dual residual is the
certificate's stationarity norm, infinite-bound rows are zeroed by a select, and the C ABI declares
the three entry points."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import LPV_CASES, lpv_qps

from cmpc import duals as D
from cmpc import structure as St

REL = 1e-12   # relative to max(1, |y_A|_inf); measured 1.2e-14 (equality part) over the 42 fixtures


def split(c):
    """(P, q, G, h, A, b) of a captured QP, and the permutation that stacks its y as [G rows; A rows]."""
    Aall, l, u = c["A"], c["l"], c["u"]
    eq = np.isfinite(l) & (l == u)
    order = np.concatenate([np.flatnonzero(~eq), np.flatnonzero(eq)])
    return (sp.csr_matrix(c["P"]), c["q"], sp.csr_matrix(Aall[~eq]), u[~eq], sp.csr_matrix(Aall[eq]), u[eq]), order


@pytest.mark.parametrize("name", LPV_CASES)
def test_recover_reproduces_the_fixture_multipliers(name):
    from oracle import qp_ipm

    for j, c in lpv_qps(name):
        args, order = split(c)
        assert np.array_equal(order, np.arange(order.size)), (name, j)   # stacked [inequalities; equalities]
        p = St.recognize(*args)
        assert p is not None, (name, j)
        m = args[2].shape[0]
        y, dua = D.recover(p, c["z"], c["y"][:m])
        assert y.shape == (1, c["y"].size) and D.ny_of(p) == c["y"].size
        np.testing.assert_array_equal(y[0, :m], c["y"][:m])          # every bound of the captured QPs is finite
        yA, ref = y[0, m:], c["y"][m:]
        rel = np.abs(yA - ref).max() / max(1.0, np.abs(ref).max())
        assert rel <= REL, (name, j, rel)
        # the slack rows of A (0 = 0): exactly 0 in the fixture and here
        ne, nx, N = p["nx"] + p["ns"], p["nx"], p["N"]
        slack = yA[: ne * (N + 1)].reshape(N + 1, ne)[:, nx:]
        assert not slack.any() and not ref[: ne * (N + 1)].reshape(N + 1, ne)[:, nx:].any()
        cert = qp_ipm.kkt_certificate(c["P"], c["q"], c["A"], c["l"], c["u"], c["z"], y[0])
        scale = max(1.0, np.abs(ref).max())
        assert abs(dua[0] - cert["stat"]) <= REL * scale, (name, j, dua[0], cert["stat"])


def _random_problem(rng, nx, nu, N, ns, mc, B):
    sl = np.array([(r % (ns + 1)) - 1 for r in range(mc)], np.int32) if ns else -np.ones(mc, np.int32)
    Qh = rng.standard_normal((nx, nx))
    return dict(nx=nx, nu=nu, N=N, ns=ns, mc=mc, Q=Qh @ Qh.T, R=np.eye(nu) * 0.5, dR=np.eye(nu) + 0.1,
                Qs=1.0 + rng.random(ns), u_ub=1.0 + rng.random(nu), u_lb=-1.0 - rng.random(nu),
                row_slack=sl, row_sign=np.where(np.arange(mc) % 2, -1, 1).astype(np.int32),
                A=rng.standard_normal((B, N, nx, nx)) * 0.5, B=rng.standard_normal((B, N, nx, nu)),
                x0=rng.standard_normal((B, nx)), u_prev=rng.standard_normal((B, nu)),
                qlin=rng.standard_normal((B, N + 1, nx)), C=rng.standard_normal((B, N, mc, nx)),
                h=rng.standard_normal((B, N, mc)))


def test_infinite_bound_rows_are_zeroed_by_a_select():
    rng = np.random.default_rng(3)
    nx, nu, N, ns, mc, B = 4, 2, 3, 3, 6, 2
    p = _random_problem(rng, nx, nu, N, ns, mc, B)
    nz = (nx + ns) * (N + 1) + 2 * nu * N
    m = N * mc + 2 * nu * N
    z = rng.standard_normal((B, nz))
    lam = rng.random((B, m))
    p["h"][:, 1, 2] = np.inf
    p["u_ub"][1] = np.inf
    p["u_lb"][0] = -np.inf
    inf = ~np.isfinite(D.bounds(p))
    assert inf.sum() == B * (1 + 2 * N)
    lam0 = np.where(inf, 0.0, lam)
    y0, d0 = D.recover(p, z, lam0)
    y1, d1 = D.recover(p, z, np.where(inf, np.nan, lam))
    assert np.isfinite(y1).all() and not y1[:, :m][inf].any()
    np.testing.assert_array_equal(y1, y0)
    np.testing.assert_array_equal(d1, d0)
    # and against the sparse reference form: dua_res is the full stationarity norm
    for a in range(B):
        P, q, G, h, A, b = St.reference_form(p, a)
        stat = P @ z[a] + q + G.T @ y1[a, :m] + A.T @ y1[a, m:]
        assert abs(np.abs(stat).max() - d1[a]) <= 1e-12 * max(1.0, np.abs(y1[a]).max())
    # a non-finite z: the NaN row
    z[1, 5] = np.nan
    y2, d2 = D.recover(p, z, lam0)
    assert np.isnan(y2[1]).all() and np.isnan(d2[1]) and np.array_equal(y2[0], y0[0]) and d2[0] == d0[0]


def test_header_declares_the_duals_entry_points():
    import ctypes as ct

    from test_abi import declared_functions

    from cmpc import _lib as L

    fns = declared_functions()
    lib = L.load()
    for need in ("cmpc_solve_mpc_batch_duals", "cmpc_solve_mpc_batch_duals_dev", "cmpc_mpc_duals_dev"):
        assert need in fns and need in L.SIGNATURES and hasattr(lib, need), need
    assert ct.sizeof(L.cmpc_mpc_duals) == 2 * ct.sizeof(ct.c_void_p)
    assert lib.cmpc_abi_version() == 6
