"""The reference structure on the GPU (include/cmpc.h): the detector kernel (csrc/mpc_lpv_detect.hip) against its
numpy statement, CMPC_FLAG_LPV routing a structured batch to the condensed kernel's compact instantiation (the
one cmpc_solve_lpv_batch runs), CMPC_FLAG_LPV_AUTO, and the adapter's ``lpv_structure`` on the captured QPs."""
import ctypes as ct

import numpy as np
import pytest

from conftest import KKT_TOL, assert_matches_optimum, lpv_qps
from lpv_level_cases import PER_AGENT, PLANTS, copy_of, osqp_args, plant, recognised, stacked, tiled

pytestmark = pytest.mark.gpu

# Complementarity of (res.x, res.y) of the routed adapter calls, relative to max(1, |y|_inf).  The bar follows the
# convention at the top of tests/test_duals_gpu.py: ten times the largest figure measured on an MI355X, rounded up
# to a power of ten, cap 1e-6.  Measured over the 36 captured QPs of the five condensed golden files (the test
# prints each): largest 2.75e-15 (lpv_n30_a3 #9), next 1.34e-15 (lpv_n10_lowspeed #3), all others <= 1.1e-15
COMP_REL = 1e-13

CONDENSED = ["lpv_n10_a2", "lpv_n30_a3", "lpv_n10_lowspeed", "lpv_n10_a1", "lpv_n20_a4"]
OUT = ("z", "kkt", "iters", "status")


def _synthetic(N, batch, nb=1, seed=0):
    """A conforming batch with random entries in every slot the compact load reads (the detector needs no solve)."""
    rng = np.random.default_rng(seed)
    mc = 4 + nb
    A = np.tile(np.eye(9), (batch, N, 1, 1))
    A[:, :, :, :3] += rng.standard_normal((batch, N, 9, 3))
    B = np.zeros((batch, N, 9, 2))
    B[:, :, :3] = rng.standard_normal((batch, N, 3, 2))
    C = np.zeros((batch, N, mc, 9))
    C[:, :, 0:2, 0] = rng.standard_normal((batch, N, 2))
    C[:, :, 2:4, 3] = rng.standard_normal((batch, N, 2))
    C[:, :, 4:, 7:9] = rng.standard_normal((batch, N, nb, 2))
    return dict(nx=9, nu=2, N=N, ns=3, mc=mc, Q=np.diag([10.0, 0, 0, 25.0, 10.0, 0, 0, 0, 0]), R=np.eye(2),
                dR=np.eye(2), Qs=np.ones(3), u_ub=np.ones(2), u_lb=-np.ones(2),
                row_slack=np.array([-1, 0, 1, 1, 2, 2, 2][:mc], np.int32),
                row_sign=np.array([1, 1, 1, 1, -1, -1, -1][:mc], np.int32), A=A, B=B, x0=np.zeros((batch, 9)),
                u_prev=np.zeros((batch, 2)), qlin=np.zeros((batch, N + 1, 9)), C=C, h=np.ones((batch, N, mc)))


def _planted(p):
    """One violation per agent in a distinct set of agents (first, both sides of a wavefront's 64, last), every kind
    of PLANTS the row count allows, at stage 0, N - 1 and in between; -0.0 where zero is required in every agent."""
    batch, N = p["A"].shape[0], p["N"]
    agents = [0, 63, 64, batch - 1, 1, 62, 2, 31, 32][: len(PLANTS)]
    assert len(set(agents)) == len(agents) and max(agents) < batch
    stages = [0, N - 1, N // 2]
    p["A"][:, :, 5, 4] = -0.0
    hit = []
    for which, a in enumerate(agents):
        if PLANTS[which][0] == "C" and PLANTS[which][1][0] >= p["mc"]:
            continue
        plant(p, a, which, stages[which % 3])
        hit.append(a)
    return hit


def _level_dev(p, ctx, level=True, count=True):
    import torch

    from cmpc import _lib as L
    from cmpc.solver import _dims, _tptr, _weights

    dev = torch.device("cuda", ctx.device)
    batch = p["A"].shape[0]
    t = {k: torch.as_tensor(np.ascontiguousarray(p[k], dtype=np.float64), device=dev) for k in ("A", "B", "C")}
    lv = torch.full((max(batch, 1),), -7, dtype=torch.int32, device=dev)
    nc = torch.full((1,), -7, dtype=torch.int32, device=dev)
    w, keep = _weights(p)
    data = L.cmpc_mpc_data(_tptr(t["A"]), _tptr(t["B"]), None, None, None, _tptr(t["C"]), None)
    s = torch.cuda.current_stream(dev)
    ctx.check(ctx.lib.cmpc_mpc_lpv_level_dev(ctx.h, ct.byref(_dims(p, batch)), ct.byref(w), ct.byref(data),
                                             _tptr(lv) if level else None, _tptr(nc) if count else None,
                                             ct.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize(dev)
    del keep
    return lv.cpu().numpy()[:batch], int(nc.cpu().numpy()[0])


def _detector_batches():
    yield "lpv_n10_a1 x130 (nb 0)", tiled(stacked("lpv_n10_a1"), 130)
    yield "lpv_n20_a4 x130 (nb 3)", tiled(stacked("lpv_n20_a4"), 130)
    yield "synthetic N 1", _synthetic(1, 70, nb=1, seed=1)
    yield "synthetic N 2", _synthetic(2, 67, nb=2, seed=2)


def test_detector_matches_the_numpy_statement(gpu_ctx):
    from cmpc import structure as St

    for tag, p in _detector_batches():
        batch = p["A"].shape[0]
        clean = St.lpv_level(p)
        assert (clean == 2).all(), tag
        lv, non = St.lpv_level_gpu(p, gpu_ctx, count=True)
        assert np.array_equal(lv, clean) and non == 0, tag
        hit = _planted(p)
        want = St.lpv_level(p)
        assert sorted(np.nonzero(want == 0)[0].tolist()) == sorted(hit), tag   # -0.0 lowered nobody
        lv, non = St.lpv_level_gpu(p, gpu_ctx, count=True)
        assert lv.dtype == np.int32 and np.array_equal(lv, want), (tag, np.nonzero(lv != want)[0])
        assert non == int((want == 0).sum()) == len(hit), tag
        lvd, nond = _level_dev(p, gpu_ctx)
        assert np.array_equal(lvd, want) and nond == non, tag
        lvd, nond = _level_dev(p, gpu_ctx, count=False)               # either output alone
        assert np.array_equal(lvd, want) and nond == -7
        lvd, nond = _level_dev(p, gpu_ctx, level=False)
        assert nond == non and (lvd == -7).all()
        q = copy_of(p)                                                # level 1, and an ineligible batch
        q["Q"][6, 6] = 3.0
        lv1, non1 = St.lpv_level_gpu(q, gpu_ctx, count=True)
        assert np.array_equal(lv1, np.where(want == 0, 0, 1)) and non1 == non
        q["Q"][0, 1] = 1.0
        for lv0, non0 in (St.lpv_level_gpu(q, gpu_ctx, count=True), _level_dev(q, gpu_ctx)):
            assert np.array_equal(lv0, np.zeros(batch, np.int32)) and non0 == batch
        print(f"{tag}: {batch} agents, nonconforming {non}: {sorted(hit)}")


def test_detector_arguments(gpu_ctx):
    from cmpc import _lib as L
    from cmpc.solver import _dims, _weights

    p = _synthetic(3, 4)
    w, keep = _weights(p)
    arrs = {k: L.f64(p[k]) for k in ("A", "B", "C")}
    lv = np.full(4, -7, np.int32)
    nc = np.full(1, -7, np.int32)
    lib, h = gpu_ctx.lib, gpu_ctx.h

    def call(d, w_, data, lv_, nc_):
        return lib.cmpc_mpc_lpv_level(h, d, w_, data, lv_, nc_)

    def data_of(**miss):
        return L.cmpc_mpc_data(*[None if miss.get(k) or k not in arrs else L.dptr(arrs[k])
                                 for k in ("A", "B", "x0", "u_prev", "qlin", "C", "h")])

    d = _dims(p, 4)
    ok = data_of()
    assert call(ct.byref(d), ct.byref(w), ct.byref(ok), L.iptr(lv), L.iptr(nc)) == L.CMPC_OK
    assert (lv == 2).all() and nc[0] == 0
    assert call(None, ct.byref(w), ct.byref(ok), L.iptr(lv), L.iptr(nc)) == L.CMPC_ERR_ARG
    assert call(ct.byref(d), None, ct.byref(ok), L.iptr(lv), L.iptr(nc)) == L.CMPC_ERR_ARG
    assert call(ct.byref(d), ct.byref(w), None, L.iptr(lv), L.iptr(nc)) == L.CMPC_ERR_ARG
    assert call(ct.byref(d), ct.byref(w), ct.byref(ok), None, None) == L.CMPC_ERR_ARG
    for k in ("A", "B", "C"):
        bad = data_of(**{k: True})
        assert call(ct.byref(d), ct.byref(w), ct.byref(bad), L.iptr(lv), L.iptr(nc)) == L.CMPC_ERR_ARG, k
        assert lib.cmpc_mpc_lpv_level_dev(h, ct.byref(d), ct.byref(w), ct.byref(bad), L.iptr(lv), L.iptr(nc),
                                          None) == L.CMPC_ERR_ARG, k
    assert lib.cmpc_mpc_lpv_level_dev(h, ct.byref(d), ct.byref(w), ct.byref(ok), None, None, None) == L.CMPC_ERR_ARG
    big = L.cmpc_mpc_dims(13, 2, 3, 3, 5, 4)      # dimension errors as cmpc_solve_mpc_batch
    assert call(ct.byref(big), ct.byref(w), ct.byref(ok), L.iptr(lv), L.iptr(nc)) == L.CMPC_ERR_UNSUPPORTED
    lv[:] = -7
    nc[:] = -7
    d0 = _dims(p, 0)                              # batch == 0: nothing launched, nothing written
    assert call(ct.byref(d0), ct.byref(w), ct.byref(ok), L.iptr(lv), L.iptr(nc)) == L.CMPC_OK
    assert lib.cmpc_mpc_lpv_level_dev(h, ct.byref(d0), ct.byref(w), ct.byref(ok), L.iptr(lv), L.iptr(nc),
                                      None) == L.CMPC_OK
    assert (lv == -7).all() and nc[0] == -7
    del keep


def _solve(p, ctx, **kw):
    from cmpc.solver import solve_mpc

    return dict(zip(OUT, solve_mpc(p, ctx, rescue=True, polish=True, **kw)))


def _same(a, b, tag):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k}")


def _break_promise(p):
    """Entries the compact kernel never reads, in agents 1 and 2."""
    q = copy_of(p)
    q["B"][1, :, 3, 0] = 0.5
    if q["A"].shape[0] > 2:
        q["A"][2, :, 4, 5] += 0.5
    return q


@pytest.mark.parametrize("name", ["lpv_n30_a3", "lpv_n10_a2"])
def test_the_promise_runs_the_compact_kernel(gpu_ctx, name):
    """With CMPC_FLAG_LPV the entries outside the pattern are not read: planting there changes nothing, bit for
    bit.  Without the flag the same plants move their agents."""
    from cmpc.solver import plan

    p = stacked(name)
    batch = p["A"].shape[0]
    assert batch >= 3 and (name != "lpv_n30_a3" or batch == 12)
    q = _break_promise(p)
    ref = _solve(p, gpu_ctx, lpv=True)
    got = _solve(q, gpu_ctx, lpv=True)
    _same(ref, got, name)
    assert (ref["status"] == 1).all(), ref["status"]
    plain = _solve(p, gpu_ctx)
    moved = _solve(q, gpu_ctx)
    dz = np.abs(moved["z"] - plain["z"]).max(axis=1)
    print(f"{name}: max|dz| of the generic path under the plants {dz[1]:.3e}, {dz[2]:.3e}; compact vs generic "
          f"{np.abs(ref['z'] - plain['z']).max():.2e}; iters {ref['iters'].tolist()} / {plain['iters'].tolist()}")
    assert dz[1] > 1e-3 and dz[2] > 1e-3, dz
    # the plan reports the compact image
    a, b = plan(p, batch, rescue=True, polish=True), plan(p, batch, rescue=True, polish=True, flags=16384)
    assert a["solver"] == b["solver"] == "condensed_v3" and b["lds_bytes"] < a["lds_bytes"], (a, b)


@pytest.mark.parametrize("name", ["lpv_n10_a2", "lpv_n30_a3"])
def test_same_bits_as_the_lpv_entry(gpu_ctx, name):
    """The builder's A, B, qlin, C, h through solve_mpc(lpv=True), with the weights as lpv_solver_const maps them,
    against PlannerLPVBatch.solve on the same inputs: the same kernel on the same data."""
    import cmpc
    from cmpc import structure as St
    from oracle import lpv_ref as LR

    g, model = LR.paper_gains(), LR.SCALED_CAR_MODEL
    tr = LR.Track.build("Highway")
    groups = {}
    for j, c in lpv_qps(name):
        groups.setdefault(c["x_last"].shape[0], []).append(c)
    for rows, cs in groups.items():
        N = cs[0]["N"]
        lim = LR.scaled_car_limits(cs[0]["vx_ref"])
        bp = cmpc.PlannerLPVBatch(g["Q"], g["Qs"], g["R"], g["dR"], N, cs[0]["dt"], tr, g["wq"], model, lim,
                                  ctx=gpu_ctx)
        xa = np.stack([c["x_agents"] for c in cs])
        xa = xa if xa.shape[2] else None
        x0, x_last, u_last, u_old, pose = (np.stack([c[k] for c in cs]) for k in
                                           ("x0", "x_last", "u_last", "u_old", "pose"))
        want = bp.solve(x0, x_last, u_last, u_old, xa, pose)
        b = bp.build(x_last, u_last, xa, pose)
        assert not b["err"].any()
        nb = 0 if xa is None else xa.shape[2]
        mc = 4 + nb
        prm = bp.prm
        p = dict(nx=9, nu=2, N=N, ns=3, mc=mc, Q=np.array(prm.Q).reshape(9, 9), R=np.array(prm.R).reshape(2, 2),
                 dR=np.array(prm.dR).reshape(2, 2), Qs=np.array(prm.Qs), u_ub=np.array([prm.max_rs, prm.max_ac]),
                 u_lb=np.array([-prm.max_ls, -prm.max_dc]), row_slack=np.array([-1, 0, 1, 1, 2, 2, 2][:mc], np.int32),
                 row_sign=np.array([1, 1, 1, 1, -1, -1, -1][:mc], np.int32), A=b["A"], B=b["B"], x0=x0,
                 u_prev=u_old, qlin=b["qlin"], C=b["C"], h=b["h"])
        assert (St.lpv_level(p) == 2).all()
        got = _solve(p, gpu_ctx, lpv=True)
        _same({k: want[k] for k in OUT}, got, f"{name} rows {rows}")
        _same(got, _solve(p, gpu_ctx, lpv="auto"), f"{name} rows {rows} auto")


def test_auto_follows_the_detector(gpu_ctx):
    p = stacked("lpv_n30_a3")
    promised = _solve(p, gpu_ctx, lpv=True)
    _same(promised, _solve(p, gpu_ctx, lpv="auto"), "conforming: auto is the promise")
    _same(promised, _solve(p, gpu_ctx, flags=16384 | 32768), "both flags: the promise")
    q = copy_of(p)
    q["B"][1, :, 3, 0] = 0.5
    from cmpc.solver import solve_mpc

    plain = solve_mpc(q, gpu_ctx, rescue=True, polish=True, duals=True)
    auto = solve_mpc(q, gpu_ctx, rescue=True, polish=True, duals=True, lpv="auto")
    for k, a, b in zip(OUT + ("y", "dua_res"), plain, auto):
        np.testing.assert_array_equal(a, b, err_msg=f"one agent off the pattern: auto is the generic path ({k})")
    assert np.abs(plain[0] - promised["z"])[1].max() > 1e-3
    # ... and with duals on a conforming batch: auto is the promise in every output
    a = solve_mpc(p, gpu_ctx, rescue=True, polish=True, duals=True, lpv=True)
    b = solve_mpc(p, gpu_ctx, rescue=True, polish=True, duals=True, lpv="auto")
    for k, u, v in zip(OUT + ("y", "dua_res"), a, b):
        np.testing.assert_array_equal(u, v, err_msg=f"duals, conforming ({k})")
    _same(promised, dict(zip(OUT, a[:4])), "duals move nothing")


def test_auto_is_refused_on_the_device_entries(gpu_ctx):
    import torch

    from cmpc import _lib as L
    from cmpc.duals import ny_of
    from cmpc.solver import nz_of, solve_mpc_dev

    p = stacked("lpv_n10_a2")
    batch = p["A"].shape[0]
    dev = torch.device("cuda", gpu_ctx.device)
    t = {k: torch.as_tensor(np.ascontiguousarray(p[k], dtype=np.float64), device=dev) for k in PER_AGENT}
    out = dict(z=torch.zeros((batch, nz_of(p)), dtype=torch.float64, device=dev),
               kkt=torch.zeros(batch, dtype=torch.float64, device=dev),
               iters=torch.zeros(batch, dtype=torch.int32, device=dev),
               status=torch.zeros(batch, dtype=torch.int32, device=dev))
    with pytest.raises(L.CmpcError) as e:
        solve_mpc_dev(p, t, out, gpu_ctx, lpv="auto")
    assert e.value.code == L.CMPC_ERR_ARG and "CMPC_FLAG_LPV_AUTO" in str(e.value)
    with pytest.raises(L.CmpcError) as e:
        solve_mpc_dev(p, t, dict(out, y=torch.zeros((batch, ny_of(p)), dtype=torch.float64, device=dev)), gpu_ctx,
                      lpv="auto")
    assert e.value.code == L.CMPC_ERR_ARG
    # the promise on the device entry: the host entry's bits (same flags: no rescue on either side)
    from cmpc.solver import solve_mpc

    solve_mpc_dev(p, t, out, gpu_ctx, lpv=True)
    torch.cuda.synchronize(dev)
    want = dict(zip(OUT, solve_mpc(p, gpu_ctx, lpv=True)))
    _same(want, {k: out[k].cpu().numpy() for k in OUT}, "device entry")


def _di_batch():
    from cmpc import scenarios as S
    from oracle import synth

    sc = S.make_di(8, 9, 2, 2)
    return synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj, np.arange(8))


@pytest.mark.parametrize("case", ["di", "n125", "generic"])
def test_flags_are_ignored_where_the_batch_is_not_eligible(gpu_ctx, case):
    from cmpc.solver import plan

    kw = {}
    if case == "di":
        p = _di_batch()
        assert tuple(int(p[k]) for k in ("nx", "nu", "N", "ns", "mc")) == (4, 2, 9, 3, 6)
    elif case == "n125":
        p = stacked("lpv_n125_a3")
        for k in PER_AGENT:
            p[k] = np.ascontiguousarray(p[k][:2])
    else:
        p = stacked("lpv_n10_a2")
        kw = dict(generic=True)
    batch = p["A"].shape[0]
    base = _solve(p, gpu_ctx, **kw)
    info = plan(p, batch, rescue=True, polish=True, **kw)
    assert info["solver"] == {"di": "condensed_v3", "n125": "riccati", "generic": "condensed"}[case]
    for lpv, bits in ((True, 16384), ("auto", 32768)):
        _same(base, _solve(p, gpu_ctx, lpv=lpv, **kw), f"{case} lpv={lpv}")
        got = plan(p, batch, rescue=True, polish=True, flags=bits, **kw)
        assert got["solver"] == info["solver"] and got["lds_bytes"] == info["lds_bytes"], (case, got, info)


@pytest.mark.parametrize("name", CONDENSED)
def test_routed_adapter_on_the_captured_qps(gpu_ctx, name):
    """Every captured QP of the condensed golden files through osqp_solve_qp(lpv_structure=True): the bars of
    test_osqp_adapter_on_reference_captured_qp, the OSQP-form KKT certificate of (res.x, res.y), and a batch call
    equal to one call per QP."""
    import cmpc
    from oracle import qp_ipm

    singles = []
    for j, (c, _) in enumerate(recognised(name)):
        res, feasible = cmpc.osqp_solve_qp(*osqp_args(c), ctx=gpu_ctx, lpv_structure=True)
        assert res.info.solver == "structured"
        assert feasible == 1 and res.info.status_val == 1, (j, res.info.status)
        assert res.info.kkt <= 1e-6 and res.info.pri_res <= 1e-6, (res.info.kkt, res.info.pri_res)
        assert_matches_optimum(res.x, c, 1e-6)
        assert res.y is not None and res.y.shape == c["y"].shape and np.isfinite(res.y).all()
        cert = qp_ipm.kkt_certificate(c["P"], c["q"], c["A"], c["l"], c["u"], res.x, res.y)
        ys = max(1.0, np.abs(res.y).max())
        print(f"{name} #{j}: stat_rel {cert['stat_rel']:.2e} prim {cert['prim']:.2e} comp/|y| {cert['comp'] / ys:.2e} "
              f"sign {cert['dual_sign']:.1e} |y| {ys:.1e} iters {res.info.iter}")
        assert cert["stat_rel"] <= KKT_TOL and cert["prim"] <= KKT_TOL, (name, j, cert)
        assert cert["dual_sign"] == 0.0, (name, j, cert)
        assert cert["comp"] <= COMP_REL * ys, (name, j, cert)
        singles.append(res)
    out = cmpc.osqp_solve_qp_batch([osqp_args(c) for c, _ in recognised(name)], ctx=gpu_ctx, lpv_structure=True)
    for one, (res, feasible) in zip(singles, out):
        assert feasible == 1 and res.info.solver == "structured"
        assert np.array_equal(res.x, one.x) and np.array_equal(res.y, one.y)
        assert res.info.iter == one.info.iter and res.info.kkt == one.info.kkt
