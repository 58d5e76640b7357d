"""The dual solution of the structured agent-QP solves on the GPU (cmpc_solve_mpc_batch_duals,
csrc/mpc_dual.hip): the kernel against its numpy statement, the OSQP-form KKT certificate of
``osqp_solve_qp``'s (res.x, res.y) on every captured reference QP, the fixtures' own multipliers where
they are unique, the polish exits, and that asking for duals moves nothing else."""
import ctypes as ct

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import KKT_TOL, LPV_CASES, golden, lpv_qps

pytestmark = pytest.mark.gpu

# Bars: ten times the largest figure measured on an MI355X, rounded up to a power of ten, never looser
# than the cap named with each (each test prints its figures).
#   kernel vs cmpc.duals.recover, |y - y_np|_inf / max(1, |y_np|_inf) and the same for dua_res, per shape:
#   y 0, 8.8e-17, 3.3e-16, 3.7e-16, 4.0e-16, 1.2e-15; dua_res 0, 0, 1.6e-16, 2.5e-16, 4.0e-16, 2.4e-16
#   -> largest 1.2e-15 (cap 1e-9)
KERNEL_REL = 1e-13
#   complementarity of (res.x, res.y) over the 42 captured QPs and the polished agents, relative to
#   max(1, |y|_inf): largest 3.4e-14 (lpv_n125_a3 #4; all others <= 2.8e-15) (cap 1e-6)
COMP_REL = 1e-12
#   res.y against the fixtures' y on the 40 strictly complementary optima, relative to max(1, |y*|_inf)
#   (|y*| reaches 1.9e7): largest 8.2e-8 (lpv_n125_a3 #4), next 5.5e-11, all others <= 2.9e-12 (cap 1e-4)
DIRECT_REL = 1e-6
# dua_res against the certificate's stat: not measured but reasoned.  Both sum, per column of the stationarity
# vector, at most nx + mc + 4 < 50 products of a coefficient (|.| < 1e2 in these QPs) with an entry of y, in
# different orders: |difference| <= 2 * 50 * 2^-53 * 1e2 * |y|_inf ~ 1e-12 |y|_inf
DUA_REL = 1e-12

SHAPES = [  # nx, nu, N, ns, mc, batch
    (1, 1, 1, 0, 0, 1),       # no stage rows, no slacks, one stage
    (4, 2, 2, 3, 6, 5),       # batch not a multiple of 4
    (9, 2, 10, 3, 5, 3),
    (12, 4, 3, 4, 16, 7),     # every maximum
    (6, 3, 50, 3, 6, 9),
    (9, 2, 125, 3, 6, 2),
]


def _random_problem(rng, nx, nu, N, ns, mc, B):
    sl = np.array([(r % (ns + 1)) - 1 for r in range(mc)], np.int32) if ns else -np.ones(mc, np.int32)
    Qh = rng.standard_normal((nx, nx))
    return dict(nx=nx, nu=nu, N=N, ns=ns, mc=mc, Q=Qh @ Qh.T, R=np.eye(nu) * 0.5, dR=np.eye(nu) + 0.1,
                Qs=1.0 + rng.random(ns), u_ub=1.0 + rng.random(nu), u_lb=-1.0 - rng.random(nu),
                row_slack=sl, row_sign=np.where(np.arange(mc) % 2, -1, 1).astype(np.int32),
                A=rng.standard_normal((B, N, nx, nx)) / np.sqrt(nx), B=rng.standard_normal((B, N, nx, nu)),
                x0=rng.standard_normal((B, nx)), u_prev=rng.standard_normal((B, nu)),
                qlin=rng.standard_normal((B, N + 1, nx)), C=rng.standard_normal((B, N, mc, nx)),
                h=rng.standard_normal((B, N, mc)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_recover(gpu_ctx, shape):
    from cmpc import duals as D

    nx, nu, N, ns, mc, B = shape
    rng = np.random.default_rng(sum(shape))
    p = _random_problem(rng, nx, nu, N, ns, mc, B)
    nz = (nx + ns) * (N + 1) + 2 * nu * N
    m = N * mc + 2 * nu * N
    if mc:
        p["h"][rng.random((B, N, mc)) < 0.2] = np.inf
    p["u_ub"][0] = np.inf
    if nu > 1:
        p["u_lb"][nu - 1] = -np.inf
    inf = ~np.isfinite(D.bounds(p))
    assert inf.any()
    z = rng.standard_normal((B, nz))
    lam = np.where(inf, np.nan, rng.random((B, m)))
    if B > 1:
        z[B - 1, nz // 2] = np.nan
    y_np, d_np = D.recover(p, z, lam)
    y, d = D.recover_gpu(p, z, lam, gpu_ctx)
    good = np.isfinite(z).all(1)
    assert good.sum() == max(B - 1, 1)
    assert np.isnan(y[~good]).all() and np.isnan(d[~good]).all()          # the NaN row, exactly
    assert np.isfinite(y[good]).all() and np.isfinite(d[good]).all()
    assert not y[good][:, :m][inf[good]].any()                            # exact zeros on infinite-bound rows
    ey = np.abs(y[good] - y_np[good]).max() / max(1.0, np.abs(y_np[good]).max())
    ed = np.abs(d[good] - d_np[good]).max() / max(1.0, np.abs(d_np[good]).max())
    print(f"shape {shape}: y rel {ey:.2e}, dua_res rel {ed:.2e} (|y| {np.abs(y_np[good]).max():.1e})")
    assert ey <= KERNEL_REL and ed <= KERNEL_REL, (ey, ed)


def _osqp_args(c):
    Aall, l, u = c["A"], c["l"], c["u"]
    eq = np.isfinite(l) & (l == u)
    return sp.csr_matrix(c["P"]), c["q"], sp.csr_matrix(Aall[~eq]), u[~eq], sp.csr_matrix(Aall[eq]), u[eq]


_SOLVED = {}


def _solved(name, gpu_ctx):
    """Every captured QP of a golden file through osqp_solve_qp, once per session."""
    from cmpc.qp import osqp_solve_qp

    if name not in _SOLVED:
        out = []
        for j, c in lpv_qps(name):
            res, feasible = osqp_solve_qp(*_osqp_args(c), ctx=gpu_ctx)
            out.append((j, c, res))
        _SOLVED[name] = out
    return _SOLVED[name]


def _certify(P, q, A, l, u, x, y, tag):
    from oracle import qp_ipm

    cert = qp_ipm.kkt_certificate(P, q, A, l, u, x, y)
    ys = max(1.0, np.abs(y).max())
    print(f"{tag}: stat_rel {cert['stat_rel']:.2e} prim {cert['prim']:.2e} comp/|y| {cert['comp'] / ys:.2e} "
          f"sign {cert['dual_sign']:.1e} |y| {ys:.1e}")
    assert cert["stat_rel"] <= KKT_TOL and cert["prim"] <= KKT_TOL, (tag, cert)
    assert cert["dual_sign"] == 0.0, (tag, cert)
    assert cert["comp"] <= COMP_REL * ys, (tag, cert)
    return cert


@pytest.mark.parametrize("name", LPV_CASES)
def test_certificate_on_the_captured_qps(gpu_ctx, name):
    """(res.x, res.y) is a KKT point of the QP as OSQP states it; needs no uniqueness of y.  N = 125 runs
    the Riccati kernel's latency mode."""
    for j, c, res in _solved(name, gpu_ctx):
        assert res.info.status_val == 1 and res.info.solver == "structured"
        assert res.y is not None and res.y.shape == c["y"].shape and np.isfinite(res.y).all()
        cert = _certify(c["P"], c["q"], c["A"], c["l"], c["u"], res.x, res.y, f"{name} #{j}")
        ys = max(1.0, np.abs(res.y).max())
        print(f"    dua_res {res.info.dua_res:.3e} vs stat {cert['stat']:.3e}: {abs(res.info.dua_res - cert['stat']) / ys:.1e} |y|")
        assert abs(res.info.dua_res - cert["stat"]) <= DUA_REL * ys, (name, j, res.info.dua_res, cert["stat"])


def test_direct_comparison_with_the_fixture_multipliers(gpu_ctx):
    """Where the certified optimum is strictly complementary (min over the inequality rows of
    max(gap, |y|) >= 1e-6) its multipliers are unique and res.y must be them."""
    skipped, worst = [], 0.0
    for name in LPV_CASES:
        for j, c, res in _solved(name, gpu_ctx):
            ineq = ~(np.isfinite(c["l"]) & (c["l"] == c["u"]))
            gap = (c["u"] - c["A"] @ c["z"])[ineq]
            if np.maximum(gap, np.abs(c["y"][ineq])).min() < 1e-6:
                skipped.append((name, j))
                continue
            rel = np.abs(res.y - c["y"]).max() / max(1.0, np.abs(c["y"]).max())
            worst = max(worst, rel)
            print(f"{name} #{j}: |y - y*| / |y*| {rel:.2e} (|y*| {np.abs(c['y']).max():.1e})")
            assert rel <= DIRECT_REL, (name, j, rel)
    print("skipped (not strictly complementary):", skipped, "worst", worst)
    assert set(skipped) <= {("lpv_n20_a4", 0), ("lpv_n125_a3", 0)}, skipped


def _polish_problems():
    d = golden("polish_lpv")
    P = {k: d[k] for k in d.files if not k.startswith("status_")}
    for k in ("nx", "nu", "N", "ns", "mc"):
        P[k] = int(P[k])
    return P, d["status_plain"]


def test_polish_exits_carry_their_multipliers(gpu_ctx):
    import cmpc
    from cmpc import structure as St

    P, st_plain = _polish_problems()
    z, kkt, it, st, y, dua = cmpc.solve_mpc(P, gpu_ctx, rescue=True, polish=True, duals=True)
    assert (st == cmpc.CMPC_SOLVED).all(), st
    assert np.isfinite(y).all() and np.isfinite(dua).all()
    floor = np.flatnonzero(st_plain == 2)
    assert floor.size
    for a in floor:
        Pm, q, G, h, A, b = St.reference_form(P, int(a))
        Aall = sp.vstack([G, A]).toarray()
        l = np.concatenate([np.full(h.size, -np.inf), b])
        u = np.concatenate([h, b])
        cert = _certify(Pm.toarray(), q, Aall, l, u, z[a], y[a], f"polish agent {a}")
        assert abs(dua[a] - cert["stat"]) <= DUA_REL * max(1.0, np.abs(y[a]).max())


def _di_population():
    from cmpc import scenarios as S
    from oracle import synth

    sc = S.make_di(96, 20, 2, 2)
    return synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj,
                            np.arange(96))


@pytest.mark.parametrize("path", ["default", "generic", "riccati", "polish_lpv"])
def test_nothing_else_moves(gpu_ctx, path):
    """z, kkt, iters, status are bit-equal with and without duals."""
    import cmpc

    if path == "polish_lpv":
        P, kw = _polish_problems()[0], dict(rescue=True, polish=True)
    else:
        P, kw = _di_population(), ({} if path == "default" else {path: True})
    base = cmpc.solve_mpc(P, gpu_ctx, **kw)
    with_duals = cmpc.solve_mpc(P, gpu_ctx, duals=True, **kw)
    for a, b in zip(base, with_duals[:4]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    st, y, dua = with_duals[3], with_duals[4], with_duals[5]
    assert (st == cmpc.CMPC_SOLVED).any()
    ok = st == cmpc.CMPC_SOLVED
    assert np.isfinite(y[ok]).all() and np.isfinite(dua[ok]).all()
    # ... and the multipliers are the solve's: stationarity to the bar z is held to (conftest's KKT_TOL)
    rel = dua[ok] / np.maximum(1.0, np.abs(y[ok]).max(1))
    print(f"{path}: {int(ok.sum())} solved, dua_res / max(1, |y|) {rel.max():.2e}")
    assert rel.max() <= KKT_TOL


def test_contract_edges(gpu_ctx):
    import cmpc
    from cmpc import _lib as L
    from cmpc import scenarios as S
    from cmpc.solver import _dims, _weights
    from oracle import synth

    P = _di_population()
    # a solve cut short holds no multipliers of the iterate it returns
    z, kkt, it, st, y, dua = cmpc.solve_mpc(P, gpu_ctx, max_iter=2, duals=True)
    assert (st != cmpc.CMPC_SOLVED).all() and np.isnan(y).all() and np.isnan(dua).all()
    # the fp32 and lane paths return none
    sc = S.make_di(8, 50, 2, 3)
    P5 = synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj, np.arange(8))
    for kw in (dict(fp32=True), dict(lane=True)):
        with pytest.raises(cmpc.CmpcError) as e:
            cmpc.solve_mpc(P5, gpu_ctx, duals=True, **kw)
        assert e.value.code == L.CMPC_ERR_UNSUPPORTED
    # batch == 0 is fine; a NULL y is an argument error
    w, keep = _weights(P)
    data = L.cmpc_mpc_data(*[L.dptr(L.f64(P[k])) for k in ("A", "B", "x0", "u_prev", "qlin", "C", "h")])
    zb = np.zeros_like(z)
    out = L.cmpc_mpc_out(L.dptr(zb), None, None, None)
    yb = np.zeros_like(y)
    lib = gpu_ctx.lib
    rc = lib.cmpc_solve_mpc_batch_duals(gpu_ctx.h, ct.byref(_dims(P, 0)), ct.byref(w), ct.byref(data), ct.byref(out),
                                        ct.byref(L.cmpc_mpc_duals(L.dptr(yb), None)), None)
    assert rc == L.CMPC_OK
    rc = lib.cmpc_solve_mpc_batch_duals(gpu_ctx.h, ct.byref(_dims(P, 96)), ct.byref(w), ct.byref(data),
                                        ct.byref(out), ct.byref(L.cmpc_mpc_duals(None, None)), None)
    assert rc == L.CMPC_ERR_ARG
    rc = lib.cmpc_solve_mpc_batch_duals(gpu_ctx.h, ct.byref(_dims(P, 96)), ct.byref(w), ct.byref(data),
                                        ct.byref(out), None, None)
    assert rc == L.CMPC_ERR_ARG
    rc = lib.cmpc_mpc_duals_dev(gpu_ctx.h, ct.byref(_dims(P, 0)), ct.byref(w), ct.byref(data), None, None,
                                ct.byref(L.cmpc_mpc_duals(L.dptr(yb), None)), None)
    assert rc == L.CMPC_OK
    del keep
