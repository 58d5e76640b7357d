"""3-D positions on the linear-model family on the device (cmpc_lin3_*, cmpc_nbr_select3_dev, cmpc_lin_rounds_create3 /
_create_table3): every kernel bit for bit against its numpy statement (cmpc.scenarios with ``iz`` in prm), and the
round handle on the stacked population — pairs of agents over one ground point, which the planar rule cannot
separate — against a host loop.  The handle tests run at cfg5's shape (nx 6, nu 3, nb 2, N 50): the stage-wise
Riccati solver, the path a 3-D double integrator has a test record on."""
import ctypes as ct

import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S
from lin3_cases import (BUILD_SHAPES, PRM, PUBLISH_SHAPE, build_instance, planted, population, publish_instance,
                        same)

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy().copy()


# ---- 1. the builder ----

def run_build(ctx, prm, own, nbr, traj, off):
    import torch
    from cmpc.rounds import lin_build_dev

    mo = own["C_own"].shape[2]
    d_own = dict(qlin_own=dev(own["qlin_own"]), C_own=dev(own["C_own"]) if mo else None,
                 h_own=dev(own["h_own"]) if mo else None)
    out = lin_build_dev(prm, d_own, dev(nbr) if nbr.shape[1] else None, dev(traj), off, ctx=ctx)
    torch.cuda.synchronize()
    return [host(t) for t in out]


@pytest.mark.parametrize("shape", BUILD_SHAPES)
def test_builder_kernel_equals_lin_rows(gpu_ctx, shape):
    prm, own, nbr, traj, off = build_instance(shape)
    nx, mo, nb, N, B, ix, iy, iz = shape
    if shape == BUILD_SHAPES[0]:                        # negative zeros in the own arrays survive the copies
        own["qlin_own"][:, ::2] = -0.0
        own["C_own"][:, :, 1] = -0.0
        own["h_own"][:, 0] = -0.0
    if shape == BUILD_SHAPES[1]:                        # agent 1's neighbour 2 (row 5: no local agent) sits on
        nbr[1] = [0, 3, 5]                              # its 3-D point at stage 1; its neighbour 1 (row 3) over its
        traj[5, 1] = traj[off + 1, 1]                   # ground point at stage 0, at another altitude
        traj[3, 0, :2] = traj[off + 1, 0, :2]
    want = S.lin_rows(prm, own, nbr, traj, off)
    got = run_build(gpu_ctx, prm, own, nbr, traj, off)
    for name, g, w in zip(("qlin", "C", "h"), got, want):
        assert same(g, w), name
    q, C, h = got
    if shape == BUILD_SHAPES[0]:
        assert np.signbit(C[:, :, 1]).all() and np.signbit(h[:, 0, :mo]).all() and np.signbit(q[:, 0]).all()
    if shape == BUILD_SHAPES[1]:
        pos = [ix, iy, iz]
        assert np.isnan(C[1, 1, mo + 2, pos]).all() and np.isnan(h[1, 1, mo + 2]) and np.isnan(q[1, 2, pos]).all()
        assert np.isnan(C).sum() == 3 and np.isnan(h).sum() == 1 and np.isnan(q).sum() == 3
        assert C[1, 0, mo + 1, ix] == 0.0 and C[1, 0, mo + 1, iy] == 0.0 and abs(C[1, 0, mo + 1, iz]) == 1.0
    else:
        assert all(np.isfinite(a).all() for a in got)


def test_builder_on_coplanar_data_equals_the_planar_kernel(gpu_ctx):
    sc = S.make_di(16, 6, 2, 3)
    lin, l3 = S.lin_of_di(sc), S.lin3_of_di(sc, 1.75)
    want = run_build(gpu_ctx, lin["prm"], lin["own"], lin["nbr"], lin["traj"], 0)
    got = run_build(gpu_ctx, l3["prm"], l3["own"], l3["nbr"], l3["traj"], 0)
    for name, g, w in zip(("qlin", "C", "h"), got, want):
        assert np.isfinite(w).all() and np.array_equal(g, w), name
    assert not got[1][:, :, 4:, 2].any()


# ---- 2. the table builder ----

def test_table_builder_equals_window_then_lin_rows(gpu_ctx):
    import torch
    from cmpc.rounds import lin_table_build_dev

    nx, nu, mo, nb, N, B, T = 6, 3, 4, 2, 4, 3, 3
    prm, _, nbr, traj, off = build_instance((nx, mo, nb, N, B, 4, 0, 2), 13)
    rng = np.random.default_rng(17)
    table = dict(A=rng.standard_normal((B, T, nx, nx)), B=rng.standard_normal((B, T, nx, nu)),
                 qlin=rng.standard_normal((B, T, nx)), C=rng.standard_normal((B, T, mo, nx)),
                 h=rng.standard_normal((B, T, mo)))
    d_table = {k: dev(v) for k, v in table.items()}
    for mode, t in ((L.CMPC_TABLE_PERIODIC, 0), (L.CMPC_TABLE_PERIODIC, 7), (L.CMPC_TABLE_HOLD, 1), (L.CMPC_TABLE_HOLD, 9)):
        A, Bm, own = S.lin_window(table, t, N, mode)     # t = 7, 9: past the table's end
        want = (A, Bm) + S.lin_rows(prm, own, nbr, traj, off)
        out = lin_table_build_dev(prm, d_table, t, N, dev(nbr), dev(traj), mode=mode, self_offset=off, ctx=gpu_ctx)
        torch.cuda.synchronize()
        for name, g, w in zip(("A", "B", "qlin", "C", "h"), out, want):
            assert np.isfinite(w).all() and host(g).tobytes() == w.tobytes(), (mode, t, name)


# ---- 3. advance and publish ----

def test_advance_and_publish_kernels(gpu_ctx):
    import torch
    from cmpc.rounds import lin_advance_dev, lin_publish_dev

    shape = PUBLISH_SHAPE
    nx, ns, nu, N, B, ix, iy, iz, n, off = shape
    prm, z, traj, _ = publish_instance()
    assert np.isnan(z[0, -1]) and np.isinf(z[1, nx]) and np.isnan(traj[off + 2, N, 2]) and 3 * (N + 1) > 3 * 64
    want = S.lin_publish(prm, z, nx, nu, ns, N, traj, self_offset=off)
    dz, dt = dev(z), dev(traj)
    for skip in ((), ("close",), ("delta",), ("not_close",), ("close", "delta", "not_close")):
        tl = dev(np.full((B, N + 1, 3), 7.0))
        close = None if "close" in skip else dev(np.full(B, -1, np.int32))
        delta = None if "delta" in skip else dev(np.full(B, 7.0))
        cnt = None if "not_close" in skip else dev(np.array([10], np.int32))
        lin_publish_dev(prm, dz, nx, nu, ns, N, dt, tl, self_offset=off, close=close, delta=delta, not_close=cnt,
                        ctx=gpu_ctx)
        torch.cuda.synchronize()
        assert same(host(tl), want[0]), skip
        assert close is None or np.array_equal(host(close), want[1]), skip
        assert delta is None or same(host(delta), want[2]), skip
        assert cnt is None or host(cnt)[0] == 10 + want[3], skip                  # added to what was there
    assert want[3] == 5 and list(want[1]) == [0, 0, 0, 0, 1, 0] and np.signbit(want[0][3, 3, 2])
    assert host(dt).tobytes() == traj.tobytes()                                   # the exchange buffer is only read
    # the advance: agents 0, 1 (a NaN in the never-copied du tail, an inf in a slack) keep all three
    rng = np.random.default_rng(3)
    x0, up, tr = rng.standard_normal((B, nx)), rng.standard_normal((B, nu)), rng.standard_normal((B, N + 1, 3))
    adv = S.lin_advance(prm, z, nx, nu, ns, N, x0, up, tr)
    d = [dev(a) for a in (x0, up, tr)]
    lin_advance_dev(prm, dz, nx, nu, ns, N, *d, ctx=gpu_ctx)
    torch.cuda.synchronize()
    for g, w, before in zip(d, adv, (x0, up, tr)):
        assert host(g).tobytes() == w.tobytes()
        assert np.array_equal(w[[0, 1]], before[[0, 1]]) and not np.array_equal(w[2:], before[2:])
    assert np.signbit(host(d[2])[3, 3, 2])


# ---- 4. the selector ----

def select(ctx, traj, nb, window=(0, 0), batch=None, off=0, with_d2=True):
    import torch
    from cmpc.rounds import select_neighbours_dev

    t = dev(traj, torch.float64)
    B = traj.shape[0] - off if batch is None else batch
    d2 = torch.full((B, nb), -1.0, dtype=torch.float64, device="cuda") if with_d2 else None
    out = select_neighbours_dev(t, nb, batch, off, window, dist2=d2, ctx=ctx)
    torch.cuda.synchronize()
    return host(out), (host(d2) if with_d2 else None)


def check_select(ctx, traj, nbs, window, batch=None, off=0):
    """Every nb of `nbs` on the device, with and without dist2, against one host selection of the longest list (a
    shorter list is its prefix: the order is total)."""
    n = traj.shape[0]
    rows = slice(off, n if batch is None else off + batch)
    ref, rd2 = S.select_neighbours(traj, max(nbs), window, rows=rows, return_dist2=True)
    for nb in nbs:
        idx, d2 = select(ctx, traj, nb, window, batch, off)
        assert idx.dtype == np.int32 and np.array_equal(idx, ref[:, :nb]), (n, nb, window)
        assert d2.tobytes() == rd2[:, :nb].tobytes(), (n, nb, window)
        assert not (idx == np.arange(n)[rows, None]).any()
        assert np.array_equal(select(ctx, traj, nb, window, batch, off, with_d2=False)[0], idx), (n, nb, window)


@pytest.mark.parametrize("window", [(0, 17), (3, 3)])
def test_selector_two_chunks_two_tiles(gpu_ctx, window):
    """n_total 130: two candidate tiles; N 17, window (0, 17): two LDS chunks, the last of two stages.  Duplicated
    points (ties, and neighbours at distance 0) and a NaN coordinate at the last stage."""
    traj = planted(population(130, 17))
    check_select(gpu_ctx, traj, (2, 4, 12), window)
    check_select(gpu_ctx, traj, (2, 4, 12), window, batch=5, off=3)          # a part-filled second workgroup
    idx, d2 = select(gpu_ctx, traj, 2, window)
    assert list(idx[1]) == [65, 129] and (d2[1] == 0.0).all()                # equal scores: the index decides
    if window == (0, 17):
        full, fd2 = select(gpu_ctx, traj, 12, window, batch=1, off=5)        # the agent with the NaN: all +inf
        assert np.isinf(fd2).all() and list(full[0]) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12]


def test_selector_side_by_side_tiles(gpu_ctx):
    """A one-stage window stages 16 tiles (2048 candidates) per step: n_total 2100 takes two steps."""
    traj = planted(population(2100, 1))
    check_select(gpu_ctx, traj, (2, 4, 12), (0, 0), batch=5, off=3)
    check_select(gpu_ctx, traj, (2,), (0, 0))
    check_select(gpu_ctx, traj, (2,), (0, 0), batch=9, off=2091)             # the population's last agents


def test_selector_uses_the_third_coordinate(gpu_ctx):
    t = np.zeros((3, 2, 3))
    t[1, :] = (0.0, 0.0, 2.0)
    t[2, :] = (1.0, 0.0, 0.0)
    assert select(gpu_ctx, t, 1)[0][0, 0] == 2 and select(gpu_ctx, t[..., :2].copy(), 1)[0][0, 0] == 1
    from cmpc import CmpcError
    with pytest.raises(CmpcError) as e:
        select(gpu_ctx, t, 3)                                                # nb >= n_total: the planar rules
    assert e.value.code == L.CMPC_ERR_ARG


# ---- 5. the handle on the stacked population ----

KEYS = ("z", "kkt", "iters", "status", "x0", "u_prev")


@pytest.fixture(scope="module")
def stacked():
    return S.make_stacked(12, 50)


def make_handle(m, ctx, **kw):
    from cmpc.rounds import LinRoundsHandle, LinTableRoundsHandle

    if "table" in m:
        return LinTableRoundsHandle(m["shared"], m["prm"], m["table"], m["x0"], m["u_prev"], m["nbr"], m["traj"],
                                    mode=m["mode"], ctx=ctx, **kw)
    return LinRoundsHandle(m["shared"], m["prm"], m["own"], m["A"], m["B"], m["x0"], m["u_prev"], m["nbr"], m["traj"],
                           ctx=ctx, **kw)


def handle_state(H):
    d = H.read()
    d["traj"] = H.get_traj()
    return d


def assert_bytes(got, want, what, keys=KEYS + ("traj",)):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def host_round(m, ctx, x0, u_prev, traj, nbr=None, t=0):
    """(lin_window ->) 3-D lin_rows -> cmpc.solve_mpc -> 3-D lin_advance: one round on the host's side of the ABI."""
    import cmpc

    sh = m["shared"]
    A, B, own = S.lin_window(m["table"], t, sh["N"], m["mode"]) if "table" in m else (m["A"], m["B"], m["own"])
    qlin, C, h = S.lin_rows(m["prm"], own, m["nbr"] if nbr is None else nbr, traj)
    z, kkt, iters, status = cmpc.solve_mpc(dict(sh, A=A, B=B, x0=x0, u_prev=u_prev, qlin=qlin, C=C, h=h), ctx)
    # the comparator alone: a finite plan, solved or solved to the inaccurate tolerance
    assert np.isfinite(z).all() and np.isin(status, (L.CMPC_SOLVED, L.CMPC_SOLVED_INACCURATE)).all(), status
    x1, u1, t1 = S.lin_advance(m["prm"], z, sh["nx"], sh["nu"], sh["ns"], sh["N"], x0, u_prev, traj)
    return dict(z=z, kkt=kkt, iters=iters, status=status, x0=x1, u_prev=u1, traj=t1)


def test_rounds_on_the_stacked_population_equal_the_host_loop(gpu_ctx, stacked):
    m = stacked
    H = make_handle(m, gpu_ctx)
    assert H.pos_dim == 3
    x0, up, traj = m["x0"], m["u_prev"], m["traj"]
    for rnd in range(3):
        want = host_round(m, gpu_ctx, x0, up, traj)
        assert H.step() == 1
        got = handle_state(H)
        assert got["traj"].shape == (12, 51, 3)
        assert_bytes(got, want, rnd)
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    assert not np.array_equal(traj[..., 2], m["traj"][..., 2])               # the plans use the altitude
    H.close()


def test_reselect_uses_the_3d_selection(gpu_ctx, stacked):
    m = stacked
    H = make_handle(m, gpu_ctx, reselect=True)
    x0, up, traj, sels = m["x0"], m["u_prev"], m["traj"], []
    for rnd in range(4):
        sel = S.select_neighbours(traj, 2)               # 3-D, on the buffer as the last exchange left it
        want = host_round(m, gpu_ctx, x0, up, traj, nbr=sel)
        assert H.step() == 1
        got = handle_state(H)
        assert np.array_equal(got["nbr"], sel), rnd
        assert_bytes(got, want, rnd)
        sels.append(sel)
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    assert any(not np.array_equal(a, b) for a, b in zip(sels, sels[1:]))      # the table changes between rounds
    H.close()


def test_consensus_step_equals_the_host_loop(gpu_ctx, stacked):
    import cmpc

    m, sh = stacked, stacked["shared"]
    nx, nu, ns, N = sh["nx"], sh["nu"], sh["ns"], sh["N"]
    co = dict(min_rounds=3, need=2, max_rounds=4, atol=0.01, rtol=1e-5)
    H = make_handle(m, gpu_ctx)
    x0, up, traj, trace = m["x0"], m["u_prev"], m["traj"], []
    while True:
        qlin, C, h = S.lin_rows(m["prm"], m["own"], m["nbr"], traj)
        z, kkt, iters, status = cmpc.solve_mpc(dict(sh, A=m["A"], B=m["B"], x0=x0, u_prev=up, qlin=qlin, C=C, h=h),
                                               gpu_ctx)
        assert np.isfinite(z).all() and np.isin(status, (L.CMPC_SOLVED, L.CMPC_SOLVED_INACCURATE)).all(), status
        traj, close, delta, count = S.lin_publish(m["prm"], z, nx, nu, ns, N, traj, atol=co["atol"], rtol=co["rtol"])
        trace.append(count)
        stop, agreed = S.consensus_stop(trace, co["min_rounds"], co["need"], co["max_rounds"])
        if stop:
            break
    x1, u1, t1 = S.lin_advance(m["prm"], z, nx, nu, ns, N, x0, up, traj)
    print("not_close", trace, "agreed", agreed, "delta max", np.nanmax(delta))
    assert H.step_consensus(1, **co) == (1, len(trace))
    assert_bytes(handle_state(H), dict(z=z, kkt=kkt, iters=iters, status=status, x0=x1, u_prev=u1, traj=t1), "step")
    c = H.consensus()
    assert c["inner_rounds"] == len(trace) and c["agreed"] is agreed and 3 <= len(trace) <= 4
    assert np.array_equal(c["not_close"], np.asarray(trace, np.int32)) and np.array_equal(c["close"], close)
    assert same(c["delta"], delta) and trace[0] > 0       # the first inner round moves away from the rollout
    H.close()


def test_table_handle_equals_the_host_loop(gpu_ctx, stacked):
    m = dict(stacked)
    own = m.pop("own")
    rep = lambda a: np.repeat(np.asarray(a, np.float64)[:, :1], 2, axis=1)   # noqa: E731
    m.update(table=dict(A=rep(m["A"]), B=rep(m["B"]), qlin=rep(own["qlin_own"]), C=rep(own["C_own"]),
                        h=rep(own["h_own"])), mode=L.CMPC_TABLE_PERIODIC)
    m["table"]["qlin"][:, 1, 3] *= 1.1                   # row 1 asks for a higher speed
    assert not np.array_equal(m["table"]["qlin"][:, 0], m["table"]["qlin"][:, 1])
    H = make_handle(m, gpu_ctx)
    assert H.pos_dim == 3
    x0, up, traj, t = m["x0"], m["u_prev"], m["traj"], 0
    for rnd in range(2):
        assert H.time == t
        want = host_round(m, gpu_ctx, x0, up, traj, t=t)
        assert H.step() == 1
        assert_bytes(handle_state(H), want, rnd)
        t = (t + 1) % 2
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    fixed = host_round(stacked, gpu_ctx, m["x0"], m["u_prev"], m["traj"])
    first = host_round(m, gpu_ctx, m["x0"], m["u_prev"], m["traj"], t=0)
    assert fixed["z"].tobytes() != first["z"].tobytes()  # the window's odd stages read row 1
    H.close()


def test_log_separation_is_three_dimensional(gpu_ctx, stacked):
    m, sh = stacked, stacked["shared"]
    H = make_handle(m, gpu_ctx, log=2, log_separation=True)
    want = host_round(m, gpu_ctx, m["x0"], m["u_prev"], m["traj"])
    assert H.step() == 1
    lg = H.log()
    near, sep2 = S.select_neighbours(want["traj"], 1, return_dist2=True)
    assert np.array_equal(lg["nearest"][0], near[:, 0]) and lg["sep2"][0].tobytes() == sep2[:, 0].tobytes()
    assert (near[:, 0] == np.arange(12) ^ 1).all() and (sep2[:, 0] > 0.3).all()        # the partner, 0.6 above or below
    flat = S.select_neighbours(want["traj"][..., :2].copy(), 1, return_dist2=True)[1]
    assert (flat[:, 0] < 1e-3).all()                     # which the planar distance calls a collision
    state, u, look = S.log_row(want["z"], sh["nx"], sh["nu"], sh["ns"], sh["N"], m["prm"]["ix"])
    assert lg["state"][0].tobytes() == state.tobytes() and lg["look_ahead"][0].tobytes() == look.tobytes()
    H.close()


def test_trajectory_buffers_have_three_columns(gpu_ctx, stacked):
    from cmpc.rounds import LinRoundsHandle

    m = stacked
    H = make_handle(m, gpu_ctx)
    assert H.get_traj().tobytes() == m["traj"].tobytes() and H.get_traj().shape == (12, 51, 3)
    moved = m["traj"].copy()
    moved[:, :, 2] += 0.05 * (np.arange(12) % 2)[:, None]
    H.set_traj(moved)
    want = host_round(m, gpu_ctx, m["x0"], m["u_prev"], moved)
    assert H.step() == 1
    assert_bytes(handle_state(H), want, "set_traj")
    with pytest.raises(ValueError):
        H.set_traj(moved[..., :2])
    H.close()
    with pytest.raises(ValueError):                      # a 2-column buffer with iz set
        make_handle(dict(m, traj=m["traj"][..., :2].copy()), gpu_ctx)
    sc = S.make_di(6, 4, 2, 3)
    P = LinRoundsHandle.of_di(sc, ctx=gpu_ctx)
    assert P.pos_dim == 2 and P.get_traj().shape == (6, 5, 2)
    with pytest.raises(ValueError):
        P.set_traj(np.zeros((6, 5, 3)))
    P.close()


def raw_create3(ctx, m, prm=None, null=()):
    """cmpc_lin_rounds_create3 on model `m` with fields replaced; returns (rc, handle)."""
    from cmpc.solver import _weights

    sh, n = m["shared"], m["x0"].shape[0]
    nb = m["nbr"].shape[1]
    cd = L.cmpc_lin_rounds_dims(n, n, 0, sh["N"], nb, 0, 1, sh["nx"], sh["nu"], sh["ns"], sh["mc"] - nb)
    p = dict(m["prm"], **(prm or {}))
    cp = L.cmpc_lin3_params(p["ix"], p["iy"], p["iz"], p["min_dist"], p["wq"])
    w, keep = _weights(sh)
    a = dict(A=L.f64(m["A"]), B=L.f64(m["B"]), x0=L.f64(m["x0"]), u_prev=L.f64(m["u_prev"]),
             qlin_own=L.f64(m["own"]["qlin_own"]), C_own=L.f64(m["own"]["C_own"]), h_own=L.f64(m["own"]["h_own"]),
             nbr=L.i32(m["nbr"]), traj=L.f64(m["traj"]))
    order = ("A", "B", "x0", "u_prev", "qlin_own", "C_own", "h_own", "nbr", "traj")
    ci = L.cmpc_lin_rounds_init(*[None if k in null else (L.iptr(a[k]) if k == "nbr" else L.dptr(a[k])) for k in order])
    co = L.opts()
    h = ct.c_void_p()
    rc = ctx.lib.cmpc_lin_rounds_create3(ctx.h, None if "prm" in null else ct.byref(cp), ct.byref(w), ct.byref(cd),
                                         ct.byref(ci), ct.byref(co), ct.byref(h))
    return rc, h


def test_create_and_device_entry_argument_errors(gpu_ctx, stacked):
    from cmpc import CmpcError

    m, lib = stacked, gpu_ctx.lib
    rc, h = raw_create3(gpu_ctx, m)
    assert rc == L.CMPC_OK and h.value
    pd = ct.c_int()
    assert lib.cmpc_lin_rounds_pos_dim(h, ct.byref(pd)) == L.CMPC_OK and pd.value == 3
    assert lib.cmpc_lin_rounds_pos_dim(h, None) == L.CMPC_ERR_ARG
    assert lib.cmpc_lin_rounds_pos_dim(None, None) == L.CMPC_ERR_ARG
    assert lib.cmpc_lin_rounds_destroy(h) == L.CMPC_OK
    nx = m["shared"]["nx"]
    for kw in (dict(prm=dict(iz=0)), dict(prm=dict(iz=1)), dict(prm=dict(iz=nx)), dict(prm=dict(iz=-1)),
               dict(prm=dict(ix=2)), dict(prm=dict(ix=1)), dict(null=("traj",)), dict(null=("prm",))):
        rc, h = raw_create3(gpu_ctx, m, **kw)
        assert rc == L.CMPC_ERR_ARG and not h.value, kw
        assert lib.cmpc_last_error(gpu_ctx.h)
    # the device entries apply the same position rules before any launch
    prm, own, nbr, traj, off = build_instance(BUILD_SHAPES[0])
    for bad in (dict(iz=0), dict(iz=1), dict(iz=6), dict(iz=-1)):
        with pytest.raises(CmpcError) as e:
            run_build(gpu_ctx, dict(prm, **bad), own, nbr, traj, off)
        assert e.value.code == L.CMPC_ERR_ARG, bad
    with pytest.raises(ValueError):                      # a 2-column buffer with iz set
        run_build(gpu_ctx, prm, own, nbr, traj[..., :2].copy(), off)


# ---- 6. the ground plane as a special case ----

def test_one_altitude_is_the_planar_handle_for_a_round(gpu_ctx):
    from cmpc.rounds import LinRoundsHandle

    sc = S.make_di(12, 50, 2, 3)
    H3 = LinRoundsHandle.of_di3(sc, 0, ctx=gpu_ctx)
    H2 = LinRoundsHandle.of_di(sc, ctx=gpu_ctx)
    assert (H3.pos_dim, H2.pos_dim) == (3, 2)
    assert H3.step() == 1 and H2.step() == 1
    a, b = handle_state(H3), handle_state(H2)
    for k in ("z", "kkt", "iters", "status"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.isfinite(b["z"]).all() and a["traj"].shape == (12, 51, 3)
    assert a["traj"][..., :2].tobytes() == b["traj"].tobytes()
    H3.close()
    H2.close()
