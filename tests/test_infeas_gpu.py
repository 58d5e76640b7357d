"""The infeasibility certificate on the GPU (csrc/mpc_infeas.hip; CMPC_FLAG_CERTIFY, cmpc_mpc_certify): the
kernel against its numpy statement (cmpc.infeas.certify) and the reference-form matrices, the solves with the
flag against the same solves without it, the osqp_solve_qp drop-in (status -3 with res.prim_inf_cert) and the
round handle's halt on -3."""
import numpy as np
import pytest

from conftest import golden, lpv_qps
from test_infeas_host import dense_reach

pytestmark = pytest.mark.gpu

# (nx, nu, N, ns, mc), row_slack
SHAPES = [((3, 2, 5, 1, 3), [-1, 0, -1]),
          ((4, 2, 10, 3, 6), [-1, 0, 1, 1, 2, -1]),
          ((12, 4, 7, 4, 16), [-1] * 16),
          ((2, 1, 33, 0, 2), [-1, -1])]     # 66 candidates: two passes of the wavefront
BATCH = 6


def problem(shape, slack, seed):
    """Seeded random, well-conditioned agents with a finite input box and h = 50 everywhere (feasible)."""
    nx, nu, N, ns, mc = shape
    rng = np.random.default_rng(seed)
    return dict(nx=nx, nu=nu, N=N, ns=ns, mc=mc, Q=np.eye(nx), R=np.eye(nu), dR=np.eye(nu), Qs=np.ones(ns),
                u_ub=np.linspace(1.0, 2.0, nu), u_lb=-np.linspace(0.5, 1.5, nu),
                row_slack=np.array(slack, np.int32), row_sign=np.ones(mc, np.int32),
                A=np.eye(nx) + 0.1 * rng.standard_normal((BATCH, N, nx, nx)) / np.sqrt(nx),
                B=0.5 * rng.standard_normal((BATCH, N, nx, nu)), x0=rng.standard_normal((BATCH, nx)),
                u_prev=np.zeros((BATCH, nu)), qlin=rng.standard_normal((BATCH, N + 1, nx)),
                C=rng.standard_normal((BATCH, N, mc, nx)), h=np.full((BATCH, N, mc), 50.0))


def plant(p, a, k, r, gap=0.3):
    p["h"][a, k - 1, r] = dense_reach(p, a, k, r) - gap


def planted(i):
    """Shape i with its unreachable rows; returns (problem, expected row per agent, -1: no certificate)."""
    shape, slack = SHAPES[i]
    nx, nu, N, ns, mc = shape
    p = problem(shape, slack, 10 + i)
    hard = [r for r in range(mc) if slack[r] < 0]
    want = -np.ones(BATCH, int)
    if N == 33:      # candidates 0, 63, 64, 65 (all rows hard: candidate q is row q), one per agent
        for a, q in enumerate((0, 63, 64, 65)):
            plant(p, a, q // mc + 1, q % mc)
            want[a] = q
    else:
        plant(p, 0, 1, hard[0])                          # stage 1
        want[0] = hard[0]
        plant(p, 1, N, hard[-1])                         # stage N
        want[1] = (N - 1) * mc + hard[-1]
        plant(p, 2, 2, hard[-1], 0.3)                    # two rows at once: the larger ratio wins ...
        plant(p, 2, N - 1, hard[0], 40.0)
        want[2] = (N - 2) * mc + hard[0]
        if len(hard) > 1:                                # ... and an exact tie (a copied row) goes to the smaller r
            p["C"][3, 2, hard[-1]] = p["C"][3, 2, hard[0]]
            plant(p, 3, 3, hard[0], 1.0)
            p["h"][3, 2, hard[-1]] = p["h"][3, 2, hard[0]]
            want[3] = 2 * mc + hard[0]
    p["x0"][5, 0] = np.nan                               # agent 4 stays feasible, agent 5 has a NaN state
    plant_nan = N // 2 + 1
    p["h"][5, plant_nan - 1, hard[0]] = -1e3
    return p, want


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_kernel_matches_the_numpy_statement_and_the_ray_verifies(gpu_ctx, i):
    from cmpc import infeas, structure

    p, want = planted(i)
    ref = infeas.certify(p)
    got = infeas.certify_gpu(p, ctx=gpu_ctx)
    assert np.array_equal(ref["row"], want), (ref["row"], want)
    assert np.array_equal(got["row"], ref["row"]), (got["row"], ref["row"])
    assert np.array_equal(got["status"], ref["status"])
    dev = 0.0
    for a in range(BATCH):
        if want[a] < 0:
            assert np.isnan(got["ray"][a]).all()
            assert np.isnan(got["margin"][a]) == np.isnan(ref["margin"][a])
            if a == 5:
                assert np.isnan(got["margin"][a])
            continue
        y = got["ray"][a]
        scale = max(1.0, np.abs(ref["ray"][a]).max())
        dev = max(dev, np.abs(y - ref["ray"][a]).max() / scale, abs(got["margin"][a] - ref["margin"][a]) / scale)
        _, _, G, h, Aeq, beq = structure.reference_form(p, a)
        res, gap = infeas.verify(G, h, Aeq, beq, y)
        print(f"shape {SHAPES[i][0]} agent {a}: row {got['row'][a]} margin {got['margin'][a]:.3e} "
              f"residual {res:.2e} gap {gap:.6f} |y|inf {np.abs(y).max():.2e}")
        assert res <= 1e-12 * np.abs(y).max() and gap < 0, (a, res, gap)
        assert (y[:h.size] >= 0).all()
    fin = np.isfinite(ref["margin"])
    dev = max(dev, np.abs(got["margin"][fin] - ref["margin"][fin]).max())
    print(f"shape {SHAPES[i][0]}: max deviation from the numpy statement {dev:.2e}")
    assert dev <= 1e-10, dev


def test_status_selects_the_agents(gpu_ctx):
    from cmpc import infeas

    p, want = planted(0)
    st = np.array([1, 2, -2, -10, -2, -10], np.int32)
    got = infeas.certify_gpu(p, st, ctx=gpu_ctx)
    ref = infeas.certify(p, st)
    assert list(got["status"]) == [1, 2, -3, -3, -2, -10] == list(ref["status"])
    assert list(got["row"]) == [-1, -1, want[2], want[3], -1, -1]
    # the skipped agents' outputs are not written: what the wrapper put there (NaN, -1) stays
    assert np.isnan(got["ray"][[0, 1]]).all() and np.isnan(got["margin"][[0, 1]]).all()
    assert np.isfinite(got["margin"][[2, 3, 4]]).all() and got["margin"][4] < 0
    # the device entry point on resident tensors: the same outputs, bit for bit
    import torch

    dev = torch.device("cuda", gpu_ctx.device)
    d = {k: torch.from_numpy(np.ascontiguousarray(p[k], dtype=np.float64)).to(dev) for k in ("A", "B", "x0", "C", "h")}
    std = torch.from_numpy(st.copy()).to(dev)
    ray = torch.full((BATCH, got["ray"].shape[1]), float("nan"), dtype=torch.float64, device=dev)
    margin = torch.full((BATCH,), float("nan"), dtype=torch.float64, device=dev)
    row = torch.full((BATCH,), -1, dtype=torch.int32, device=dev)
    infeas.certify_dev(p, d, std, ray, margin, row, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert np.array_equal(std.cpu().numpy(), got["status"]) and np.array_equal(row.cpu().numpy(), got["row"])
    assert np.array_equal(ray.cpu().numpy(), got["ray"], equal_nan=True)
    assert np.array_equal(margin.cpu().numpy(), got["margin"], equal_nan=True)


def _di_with_an_infeasible_and_a_nan_agent():
    from cmpc import scenarios as S
    from oracle import synth

    sc = S.make_di(8, 10, 2, 2)
    P = synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj, np.arange(8))
    H = dict(P)
    H["h"] = P["h"].copy()
    H["h"][0, :, 0] = -50.0          # min speed above the reachable range: hard-infeasible
    H["x0"] = P["x0"].copy()
    H["x0"][1, 0] = np.nan
    return H


@pytest.mark.parametrize("path", [dict(), dict(generic=True), dict(riccati=True), dict(rescue=True, polish=True)],
                         ids=["default", "generic", "riccati", "rescue_polish"])
def test_solve_with_the_flag(gpu_ctx, path):
    """Status -3 for the hard-infeasible agent behind every solver path; everything else bit for bit what the
    same call returns without the flag."""
    import cmpc

    H = _di_with_an_infeasible_and_a_nan_agent()
    z0, k0, i0, s0 = cmpc.solve_mpc(H, gpu_ctx, max_iter=40, **path)
    z, kkt, it, st = cmpc.solve_mpc(H, gpu_ctx, max_iter=40, certify=True, **path)
    assert s0[0] != cmpc.CMPC_PRIMAL_INFEASIBLE
    assert st[0] == cmpc.CMPC_PRIMAL_INFEASIBLE, st
    assert st[1] not in (1, 2, -3), st
    assert (st[2:] == 1).all(), st
    assert np.array_equal(z, z0, equal_nan=True) and np.array_equal(kkt, k0, equal_nan=True)
    assert np.array_equal(it, i0) and np.array_equal(st[1:], s0[1:])


def test_flag_bits(gpu_ctx):
    import cmpc
    from cmpc import _lib as L

    H = _di_with_an_infeasible_and_a_nan_agent()
    _, _, _, st = cmpc.solve_mpc(H, gpu_ctx, max_iter=40, flags=4096)
    assert st[0] == -3
    with pytest.raises(cmpc.CmpcError) as ei:
        cmpc.solve_mpc(H, gpu_ctx, max_iter=40, flags=2)
    assert ei.value.code == L.CMPC_ERR_ARG
    # the device entry: the same statuses, and the argument checks of the certificate entry points
    import ctypes as ct

    lib = gpu_ctx.lib
    assert lib.cmpc_mpc_certify(gpu_ctx.h, None, None, None, None, None) == L.CMPC_ERR_ARG
    from cmpc.solver import _dims, _weights

    w, keep = _weights(H)
    arrs = [L.f64(H[k]) for k in ("A", "B", "x0", "u_prev", "qlin", "C", "h")]
    data = L.cmpc_mpc_data(*[L.dptr(a) for a in arrs])
    assert lib.cmpc_mpc_certify(gpu_ctx.h, ct.byref(_dims(H, 8)), ct.byref(w), ct.byref(data), None,
                                None) == L.CMPC_ERR_ARG
    assert lib.cmpc_mpc_certify(gpu_ctx.h, ct.byref(_dims(H, 0)), ct.byref(w), ct.byref(data), None,
                                ct.byref(L.cmpc_mpc_cert(None, None, None))) == L.CMPC_OK


def test_solve_mpc_dev_with_the_flag(gpu_ctx):
    import torch

    import cmpc

    H = _di_with_an_infeasible_and_a_nan_agent()
    dev = torch.device("cuda", gpu_ctx.device)
    d = {k: torch.from_numpy(np.ascontiguousarray(H[k], dtype=np.float64)).to(dev) for k in cmpc.solver.PER_AGENT}
    outs = []
    for certify in (False, True):
        out = dict(z=torch.zeros((8, cmpc.nz_of(H)), dtype=torch.float64, device=dev),
                   kkt=torch.zeros(8, dtype=torch.float64, device=dev),
                   iters=torch.zeros(8, dtype=torch.int32, device=dev),
                   status=torch.zeros(8, dtype=torch.int32, device=dev))
        cmpc.solve_mpc_dev(H, d, out, gpu_ctx, max_iter=40, certify=certify)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
    a, b = outs
    assert a["status"][0] != -3 and b["status"][0] == -3 and np.array_equal(a["status"][1:], b["status"][1:])
    assert np.array_equal(a["z"], b["z"], equal_nan=True) and np.array_equal(a["iters"], b["iters"])


def _osqp_args(c):
    """(P, q, G, h, A, b) as PlannerLPV.solve passes them (tests/test_qp_gpu.py)."""
    import scipy.sparse as sp

    Aall, l, u = c["A"], c["l"], c["u"]
    eq = np.isfinite(l) & (l == u)
    return (sp.csr_matrix(c["P"]), c["q"], sp.csr_matrix(Aall[~eq]), u[~eq], sp.csr_matrix(Aall[eq]), u[eq])


def test_drop_in_reports_primal_infeasible_with_its_certificate(gpu_ctx):
    import cmpc
    from cmpc import infeas, structure

    _, c = next(iter(lpv_qps("lpv_n30_a3")))
    P, q, G, h, A, b = _osqp_args(c)
    N = int(c["N"])
    mc = (G.shape[0] - 4 * N) // N
    # the unmodified QP: status 1, x what the structured solve gives without the flag, no certificate
    res0, feas0 = cmpc.osqp_solve_qp(P, q, G, h, A, b, ctx=gpu_ctx)
    z0 = cmpc.solve_mpc(structure.recognize(P, q, G, h, A, b), gpu_ctx, rescue=True, polish=True)[0][0]
    assert res0.info.status_val == 1 and feas0 == 1 and res0.prim_inf_cert is None
    assert np.array_equal(res0.x, z0)
    hb = np.array(h, float)
    hb[(5 - 1) * mc + 0] = -50.0     # stage 5's minimum-speed row
    res, feasible = cmpc.osqp_solve_qp(P, q, G, hb, A, b, ctx=gpu_ctx)
    assert res.info.solver == "structured"
    assert res.info.status_val == -3 and res.info.status == "primal infeasible" and feasible == 0
    y = res.prim_inf_cert
    assert y is not None and y.shape == (G.shape[0] + A.shape[0],)
    r, gap = infeas.verify(G, hb, A, b, y)
    print(f"drop-in: residual {r:.2e} gap {gap:.4f} |y|inf {np.abs(y).max():.2e}")
    assert r <= 1e-12 * np.abs(y).max() and gap < 0
    # the dense path keeps its own -3 and carries no ray (x <= -1 and x >= 1)
    rd, fd = cmpc.osqp_solve_qp_batch([(np.eye(1), np.zeros(1), np.array([[1.0], [-1.0]]), np.array([-1.0, -1.0]),
                                        None, None)], ctx=gpu_ctx, max_iter=60)[0]
    assert rd.info.solver == "dense" and rd.info.status_val == -3 and fd == 0 and rd.prim_inf_cert is None


def _handle(ctx, sys_lim, certify):
    import cmpc
    from cmpc.rounds import LPVRoundsHandle
    from oracle import lpv_ref as R

    d = golden("lpv_n30_a3")
    N, n, dt = int(d["N"]), int(d["n_agents"]), float(d["dt"])
    g = R.paper_gains()
    bp = cmpc.PlannerLPVBatch(g["Q"], g["Qs"], g["R"], g["dR"], N, dt, R.Track.build("Highway"), g["wq"],
                              R.SCALED_CAR_MODEL, sys_lim, ctx=ctx, certify=certify)
    sel = sorted([j for j in range(len(d["step"])) if d["step"][j] == 0], key=lambda j: d["agent"][j])
    H = LPVRoundsHandle(bp, d["x0"][sel].copy(), np.stack([d[f"x_last_{j}"] for j in sel]),
                        np.stack([d[f"u_last_{j}"] for j in sel]),
                        np.array(R.neighbour_lists(n), np.int32).reshape(n, n - 1),
                        u_old=d["u_old"][sel].copy(), traj=d["pose"][sel].copy())
    return H, n


def test_round_handle_halts_on_primal_infeasible(gpu_ctx):
    from cmpc.planner import DEFAULT_LIMITS

    H, n = _handle(gpu_ctx, {**DEFAULT_LIMITS, "min_vel": 50.0}, True)
    assert H.step(3) == (1, n)
    assert (H.read()["status"] == -3).all()
    H.close()
    # the default limits: the flag changes nothing
    runs = []
    for certify in (False, True):
        H, n = _handle(gpu_ctx, DEFAULT_LIMITS, certify)
        done = H.step(3)
        r = H.read()
        runs.append((done, r["status"].copy(), r["z"].copy()))
        H.close()
    assert runs[1][0] == (3, 0), runs[1][0]
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][2], runs[1][2], equal_nan=True)
