"""Time-varying linear-model rounds on the device (cmpc_lin_table_build_dev / _round_dev,
cmpc_lin_rounds_create_table / _get_time / _set_time / _table_write): the one-launch table builder against its numpy
statement (lin_window, then lin_rows of that window), the double integrator as the one-row table against the
fixed-window handle (byte for byte), a 9-state model whose dynamics, reference and bound move along the table
against a host loop, the handle's behaviour and the argument errors."""
import ctypes as ct

import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S

pytestmark = pytest.mark.gpu

HOLD, PERIODIC = L.CMPC_TABLE_HOLD, L.CMPC_TABLE_PERIODIC


def dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy().copy()


def same(a, b):
    """Finite entries bit for bit, NaNs in the same places (their payloads differ between host and device)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and \
        np.where(nan, 0.0, a).tobytes() == np.where(nan, 0.0, b).tobytes()


# ---- 1. the builder kernel against lin_window + lin_rows ----

# (nx, nu, mo, nb, N, batch, ix, iy, T, mode, t): plain; the window straddles the table's end; wholly past it; wraps
# three times; no own rows (NULL C / h) and T = 1; no neighbours; more stages than the workgroup has lanes
BUILD_SHAPES = [(4, 2, 4, 2, 3, 5, 0, 1, 6, HOLD, 0), (4, 2, 4, 2, 3, 5, 0, 1, 6, HOLD, 4),
                (4, 2, 4, 2, 3, 5, 0, 1, 6, HOLD, 9), (9, 2, 4, 3, 10, 3, 7, 8, 3, PERIODIC, 2),
                (12, 4, 0, 1, 1, 1, 11, 0, 1, HOLD, 0), (6, 3, 2, 0, 4, 2, 0, 1, 5, PERIODIC, 4),
                (4, 2, 4, 2, 70, 2, 0, 1, 75, HOLD, 3)]


def build_instance(shape, seed):
    nx, nu, mo, nb, N, B, ix, iy, T, mode, t = shape
    rng = np.random.default_rng(seed)
    n, off = B + 3, 1                                   # local agents: rows 1 .. B of the exchange buffer
    table = dict(A=rng.standard_normal((B, T, nx, nx)), B=rng.standard_normal((B, T, nx, nu)),
                 qlin=rng.standard_normal((B, T, nx)), C=rng.standard_normal((B, T, mo, nx)) if mo else None,
                 h=rng.standard_normal((B, T, mo)) if mo else None)
    traj = rng.standard_normal((n, N + 1, 2))
    nbr = np.zeros((B, nb), np.int32)
    for b in range(B):
        nbr[b] = rng.permutation([j for j in range(n) if j != off + b])[:nb]
    return dict(ix=ix, iy=iy, min_dist=0.25, wq=5.0), table, nbr, traj, off


def dev_table(table):
    return {k: None if v is None else dev(v) for k, v in table.items()}


@pytest.mark.parametrize("shape", BUILD_SHAPES)
def test_table_builder_equals_window_then_lin_rows(gpu_ctx, shape):
    import torch
    from cmpc.rounds import lin_table_build_dev

    nx, nu, mo, nb, N, B, ix, iy, T, mode, t = shape
    prm, table, nbr, traj, off = build_instance(shape, 13)
    if shape == BUILD_SHAPES[0]:                        # negative zeros in every table array survive the gather
        table["A"][:, :, 1] = -0.0
        table["B"][:, ::2, :, 0] = -0.0
        table["qlin"][:, ::2] = -0.0
        table["C"][:, :, 1] = -0.0
        table["h"][:, 1] = -0.0
        table["A"][0, 2, 0, 0] = np.nan                 # and a NaN stays a NaN, where it was
    A_w, B_w, own = S.lin_window(table, t, N, mode)
    want = (A_w, B_w) + S.lin_rows(prm, own, nbr, traj, off)
    got = lin_table_build_dev(prm, dev_table(table), t, N, dev(nbr) if nb else None, dev(traj), mode, off, ctx=gpu_ctx)
    torch.cuda.synchronize()
    got = [host(g) for g in got]
    for name, g, w in zip(("A", "B", "qlin", "C", "h"), got, want):
        assert same(g, w), name
    A, Bm, q, C, h = got
    if shape == BUILD_SHAPES[0]:
        assert np.signbit(A[:, :, 1]).all() and np.signbit(Bm[:, 0, :, 0]).all() and np.signbit(Bm[:, 2, :, 0]).all()
        assert np.signbit(q[:, 0]).all() and np.signbit(C[:, :, 1]).all() and np.signbit(h[:, 0, :mo]).all()
        assert np.isnan(A).sum() == 1 and np.isnan(A[0, 2, 0, 0])
        assert all(np.isfinite(a).all() for a in got[1:])
    else:
        assert all(np.isfinite(a).all() for a in got)


# ---- 2. the double integrator is the special case ----

KEYS = ("z", "kkt", "iters", "status", "x0", "u_prev")


def handle_state(H):
    d = H.read()
    d["traj"] = H.get_traj()
    return d


def assert_bytes(got, want, what, keys=KEYS + ("traj",)):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("shape,rounds,lpt", [((64, 10, 2, 2), 4, False), ((32, 50, 2, 3), 2, True)])
def test_rounds_of_the_one_row_table_equal_the_fixed_window_handle(gpu_ctx, shape, rounds, lpt):
    """lin_of_di's arrays are constant over stages, so the T = 1 HOLD table is the double integrator again; the
    second shape runs the stage-wise Riccati solver, with the launch order."""
    from cmpc.rounds import LinRoundsHandle, LinTableRoundsHandle

    sc = S.make_di(*shape)
    F = LinRoundsHandle.of_di(sc, ctx=gpu_ctx, lpt=lpt)
    H = LinTableRoundsHandle.of_di(sc, ctx=gpu_ctx, lpt=lpt)
    assert H.T == 1 and H.time == 0
    for rnd in range(rounds):
        assert F.step() == 1 and H.step() == 1
        want = handle_state(F)
        assert_bytes(handle_state(H), want, rnd, KEYS + ("traj", "nbr"))
        assert np.isfinite(want["z"]).all() and (want["iters"] > 0).all()
        assert H.time == 0                               # HOLD: min(t + 1, T - 1)
    F.close()
    H.close()


# ---- 3. a time-varying model against the host loop ----

def make_ltv_table(T, n=12, N=10, nb=2, seed=7):
    """test_lin_rounds_gpu.make_ltv with a table of T stages in place of its N-stage window: 12 agents on the
    three-lane road with a 9-state model, x = [v_x, v_y, c2, e_y, c4, c5, c6, X, Y], u = (a_y, a_x); A_tau = I + dt
    (kinematics + seeded perturbation), B_tau likewise.  The own data move along the table: the reference speed
    rises (qlin[:, tau, 0] = -10 (3 + 0.05 tau)) and the speed bound tightens (h[:, tau, 1] = 5.5 - 0.02 tau)."""
    rng = np.random.default_rng(seed)
    nx, nu, ns, dt = 9, 2, 3, S.DT
    Ac = np.zeros((nx, nx))
    Ac[7, 0] = Ac[8, 1] = Ac[3, 1] = 1.0                # X' = v_x, Y' = v_y, e_y' = v_y
    for c in (2, 4, 5, 6):
        Ac[c, c] = -2.0                                  # the spare states decay
    Bc = np.zeros((nx, nu))
    Bc[0, 1] = Bc[1, 0] = 1.0
    Bc[2, 0] = Bc[4, 1] = 0.1
    A = np.eye(nx) + dt * (Ac + 0.02 * rng.standard_normal((n, T, nx, nx)))
    B = dt * (Bc + 0.02 * rng.standard_normal((n, T, nx, nu)))
    i = np.arange(n)
    lane = np.array([S.LANES[k % 3] for k in i])
    x0 = np.zeros((n, nx))
    x0[:, 0] = rng.uniform(1.0, 1.6, n)
    x0[:, 3] = rng.uniform(-0.05, 0.05, n)
    x0[:, 7] = 0.5 * (i // 3) + rng.uniform(-0.05, 0.05, n)
    x0[:, 8] = lane + x0[:, 3]
    x0[:, [2, 4, 5, 6]] = 0.01 * rng.standard_normal((n, 4))
    k = np.arange(N + 1)[None, :]
    traj = np.stack([x0[:, 7:8] + k * dt * x0[:, 0:1], x0[:, 8:9] + 0 * k], axis=-1)
    Q = np.diag([10.0, 1.0, 0.1, 25.0, 0.1, 0.1, 0.1, 0.0, 0.0])
    shared = dict(nx=nx, nu=nu, N=N, ns=ns, mc=4 + nb, Q=Q, R=np.zeros((nu, nu)), dR=50.0 * np.eye(nu),
                  Qs=np.full(3, 1e7), u_ub=np.array([5.0, 5.0]), u_lb=np.array([-5.0, -10.0]),
                  row_slack=np.array([-1, 0, 1, 1] + [2] * nb, np.int32),
                  row_sign=np.array([1, 1, 1, 1] + [-1] * nb, np.int32))
    tau = np.arange(T)
    C = np.zeros((n, T, 4, nx))
    C[:, :, 0, 0], C[:, :, 1, 0], C[:, :, 2, 3], C[:, :, 3, 3] = -1.0, 1.0, 1.0, -1.0
    h = np.broadcast_to(np.array([-0.0, 5.5, 0.75, 0.75]), (n, T, 4)).copy()
    h[:, :, 1] = 5.5 - 0.02 * tau
    qlin = np.zeros((n, T, nx))
    qlin[:, :, 0] = -10.0 * (3.0 + 0.05 * tau)
    return dict(shared=shared, prm=dict(ix=7, iy=8, min_dist=0.25, wq=5.0), table=dict(A=A, B=B, qlin=qlin, C=C, h=h),
                T=T, x0=x0, u_prev=np.zeros((n, nu)), nbr=S.nearest_neighbours(x0[:, 7:9], nb), traj=traj)


def table_handle(m, ctx, mode, **kw):
    from cmpc.rounds import LinTableRoundsHandle

    return LinTableRoundsHandle(m["shared"], m["prm"], m["table"], m["x0"], m["u_prev"], m["nbr"], m["traj"], mode=mode,
                                ctx=ctx, **kw)


def host_round(m, ctx, mode, t, x0, u_prev, traj, nbr=None, table=None):
    """lin_window -> lin_rows -> cmpc.solve_mpc -> lin_advance: one round at time t on the host's side of the ABI."""
    import cmpc

    sh = m["shared"]
    A, B, own = S.lin_window(m["table"] if table is None else table, t, sh["N"], mode)
    qlin, C, h = S.lin_rows(m["prm"], own, m["nbr"] if nbr is None else nbr, traj)
    P = dict(sh, A=A, B=B, x0=x0, u_prev=u_prev, qlin=qlin, C=C, h=h)
    z, kkt, iters, status = cmpc.solve_mpc(P, ctx)
    x1, u1, t1 = S.lin_advance(m["prm"], z, sh["nx"], sh["nu"], sh["ns"], sh["N"], x0, u_prev, traj)
    return dict(z=z, kkt=kkt, iters=iters, status=status, x0=x1, u_prev=u1, traj=t1)


def next_time(t, T, mode):
    return (t + 1) % T if mode == PERIODIC else min(t + 1, T - 1)


@pytest.fixture(scope="module")
def ltv14():
    return make_ltv_table(14)


# the last rounds run past the table's end; the window is longer than the table; a short ring
@pytest.mark.parametrize("T,mode,rounds", [(14, HOLD, 6), (7, PERIODIC, 6), (3, PERIODIC, 5)])
def test_rounds_of_a_time_varying_table_equal_the_host_loop(gpu_ctx, ltv14, T, mode, rounds):
    from cmpc.rounds import LinRoundsHandle

    m = ltv14 if T == 14 else make_ltv_table(T)
    sh = m["shared"]
    assert not np.array_equal(m["table"]["A"][:, 0], m["table"]["A"][:, 1])          # time-varying
    H = table_handle(m, gpu_ctx, mode)
    # the parent's handle: the t = 0 window in every round
    A0, B0, own0 = S.lin_window(m["table"], 0, sh["N"], mode)
    F = LinRoundsHandle(sh, m["prm"], own0, A0, B0, m["x0"], m["u_prev"], m["nbr"], m["traj"], ctx=gpu_ctx)
    x0, up, traj, t = m["x0"], m["u_prev"], m["traj"], 0
    for rnd in range(rounds):
        assert H.time == t
        want = host_round(m, gpu_ctx, mode, t, x0, up, traj)
        assert (want["status"] == L.CMPC_SOLVED).all(), (rnd, want["status"])    # the comparator alone
        assert H.step() == 1
        got = handle_state(H)
        assert_bytes(got, want, rnd)
        t = next_time(t, T, mode)
        if rnd <= 2:
            assert F.step() == 1
            fixed = F.read()["z"]
            # round 0 plans on the same window; by round 2 the window has to have moved
            assert (fixed.tobytes() == got["z"].tobytes()) == (rnd == 0), rnd
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    assert H.time == t and (mode == PERIODIC or t == min(rounds, T - 1))
    H.close()
    F.close()


# ---- 4. behaviour ----

def test_set_time_moves_the_window(gpu_ctx, ltv14):
    from cmpc import CmpcError

    m = ltv14
    H = table_handle(m, gpu_ctx, HOLD, t0=2)
    assert H.time == 2
    H.set_time(5)
    assert H.time == 5
    want = host_round(m, gpu_ctx, HOLD, 5, m["x0"], m["u_prev"], m["traj"])
    assert H.step() == 1
    assert_bytes(handle_state(H), want, "t = 5")
    assert H.time == 6
    H.set_time(13)                                       # the last stage: HOLD stays there
    assert H.step() == 1 and H.time == 13
    for t in (-1, 14, 1 << 30):
        with pytest.raises(CmpcError) as e:
            H.set_time(t)
        assert e.value.code == L.CMPC_ERR_ARG and H.time == 13
    H.close()


def test_write_table_changes_exactly_the_rounds_that_read_the_rows(gpu_ctx, ltv14):
    """A PERIODIC table as a ring: rows 0, 1 are consumed after two rounds and overwritten; the windows at t = 2, 3
    (rows 2..12, 3..13) do not read them, the window at t = 4 reads row 0.  Then a write of qlin alone."""
    m = ltv14
    rng = np.random.default_rng(21)
    H = table_handle(m, gpu_ctx, PERIODIC)
    U = table_handle(m, gpu_ctx, PERIODIC)               # the unedited ring
    assert H.step(2) == 2 and U.step(2) == 2 and H.time == 2
    s = handle_state(H)
    assert_bytes(handle_state(U), s, "before the write")
    ed = {k: v.copy() for k, v in m["table"].items()}
    ed["A"][:, :2] += S.DT * 0.02 * rng.standard_normal(ed["A"][:, :2].shape)
    ed["B"][:, :2] += S.DT * 0.02 * rng.standard_normal(ed["B"][:, :2].shape)
    ed["qlin"][:, :2, 0] = -10.0 * 3.3
    ed["C"][:, :2, 2, 1] = 0.125
    ed["h"][:, :2, 1] = 5.4
    H.write_table(0, **{k: v[:, :2] for k, v in ed.items()})
    x0, up, traj = s["x0"], s["u_prev"], s["traj"]
    for t in (2, 3, 4):
        want = host_round(m, gpu_ctx, PERIODIC, t, x0, up, traj, table=ed)
        assert H.step() == 1 and U.step() == 1
        got, plain = handle_state(H), handle_state(U)
        assert_bytes(got, want, t)
        assert (got["z"].tobytes() == plain["z"].tobytes()) == (t < 4), t
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    U.close()
    # a partial write: the cost rows the next window starts on, and nothing else
    assert H.time == 5
    before = dict(ed, qlin=ed["qlin"].copy())
    ed["qlin"][:, 5:7, 0] = -10.0 * 2.9
    H.write_table(5, qlin=ed["qlin"][:, 5:7])
    want = host_round(m, gpu_ctx, PERIODIC, 5, x0, up, traj, table=ed)
    assert H.step() == 1
    assert_bytes(handle_state(H), want, "qlin alone")
    old = host_round(m, gpu_ctx, PERIODIC, 5, x0, up, traj, table=before)
    assert old["z"].tobytes() != want["z"].tobytes()
    with pytest.raises(ValueError):
        H.write_table(0, A=ed["A"][:, :2], qlin=ed["qlin"][:, :3])           # two counts
    with pytest.raises(ValueError):
        H.write_table(0, h=ed["h"][:, :2, :3])
    H.close()


def test_write_of_the_model_withdraws_the_time_invariance_promise(gpu_ctx):
    """The one-row-repeated table of the double integrator passes CMPC_FLAG_LTI's test at create; after a write
    that carries A the solver must read every stage of the window again."""
    from cmpc.rounds import LinTableRoundsHandle

    sc = S.make_di(16, 10, 2, 2)
    lin = S.lin_table_of_di(sc, 3)
    H = LinTableRoundsHandle.of_di(sc, T=3, ctx=gpu_ctx, lpt=False)
    m = dict(shared=sc.shared, prm=lin["prm"], table=lin["table"], nbr=sc.nbr)
    ed = dict(lin["table"])
    ed["A"] = ed["A"].copy()
    ed["A"][:, 1:, 0, 2] *= 0.9                           # rows 1, 2: another model than row 0
    H.write_table(1, A=ed["A"][:, 1:])
    want = host_round(m, gpu_ctx, HOLD, 0, sc.x0, sc.u_prev, sc.traj, table=ed)
    stale = host_round(m, gpu_ctx, HOLD, 0, sc.x0, sc.u_prev, sc.traj)
    assert want["z"].tobytes() != stale["z"].tobytes() and np.isfinite(want["z"]).all()
    assert H.step() == 1
    assert_bytes(handle_state(H), want, "after the write")
    H.close()


def test_state_history_log_and_reselect_as_on_the_fixed_window_handle(gpu_ctx, ltv14):
    m, sh = dict(ltv14), ltv14["shared"]
    p = m["traj"][:, 0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    m["nbr"] = np.argsort(-d2, axis=1, kind="stable")[:, :2].astype(np.int32)    # the farthest: a valid table
    H = table_handle(m, gpu_ctx, HOLD, reselect=True, history=2, log=2)
    sel = S.select_neighbours(m["traj"], 2)
    assert (m["nbr"] != sel).any(axis=1).all()
    r0 = host_round(m, gpu_ctx, HOLD, 0, m["x0"], m["u_prev"], m["traj"], nbr=sel)
    assert H.step() == 1
    got = handle_state(H)
    assert np.array_equal(got["nbr"], sel)
    assert_bytes(got, r0, "reselect")
    # the measured state replaces the predicted one; the window still moves on
    x0 = r0["x0"].copy()
    x0[:, 0] += 0.05
    up = r0["u_prev"] + 0.01
    H.set_state(x0, up)
    sel = S.select_neighbours(r0["traj"], 2)
    r1 = host_round(m, gpu_ctx, HOLD, 1, x0, up, r0["traj"], nbr=sel)
    assert H.step() == 1 and H.time == 2
    assert_bytes(handle_state(H), r1, "set_state")
    # the log's rows are log_row with look_col = ix, and the history ring holds both rounds
    assert H.log_range() == (0, 2)
    lg, hist = H.log(), H.history(0, 2)
    for i, r in enumerate((r0, r1)):
        state, u, look = S.log_row(r["z"], sh["nx"], sh["nu"], sh["ns"], sh["N"], m["prm"]["ix"])
        assert lg["state"][i].tobytes() == state.tobytes() and lg["u"][i].tobytes() == u.tobytes()
        assert lg["look_ahead"][i].tobytes() == look.tobytes() and (look > 0).all()
        for k in ("kkt", "iters", "status"):
            assert lg[k][i].tobytes() == r[k].tobytes() and hist[k][i].tobytes() == r[k].tobytes(), (i, k)
    H.close()


# ---- 5. argument errors ----

SENTINEL = 7.0
OUTPUTS = ("A", "B", "qlin", "C", "h", "z", "x0", "u_prev", "traj_local", "kkt")


def dev_args(prm=None, dims=None, tdims=None):
    """Valid device arguments of cmpc_lin_table_build_dev / _round_dev on a (4, 2, 3) model with a 5-row table,
    fields replaced; every output holds the sentinel."""
    import torch
    from cmpc.solver import _weights

    p = dict(ix=0, iy=1, min_dist=0.25, wq=5.0)
    p.update(prm or {})
    d = dict(batch=2, N=3, nb=2, self_offset=0, nx=4, mo=4)
    d.update(dims or {})
    td = dict(T=5, mode=HOLD)
    td.update(tdims or {})
    B, N, nx, nu, ns, mc, T = 2, 3, 4, 2, 3, 6, 5
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")                     # noqa: E731
    s = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")            # noqa: E731
    w, keep = _weights(dict(S.di_shared(2, N, 2)))
    traj = z(4, N + 1, 2)
    traj[:] = torch.arange(4, device="cuda", dtype=torch.float64)[:, None, None]                 # distinct points
    return dict(prm=L.cmpc_lin_params(p["ix"], p["iy"], p["min_dist"], p["wq"]),
                dims=L.cmpc_lin_dims(*[d[k] for k in ("batch", "N", "nb", "self_offset", "nx", "mo")]),
                tdims=L.cmpc_lin_table_dims(td["T"], td["mode"]), nu=nu, t=0,
                nbr=torch.ones((B, 2), dtype=torch.int32, device="cuda"), tA=z(B, T, nx, nx), tB=z(B, T, nx, nu),
                tq=z(B, T, nx), tC=z(B, T, 4, nx), th=z(B, T, 4), traj_all=traj, A=s(B, N, nx, nx), B=s(B, N, nx, nu),
                qlin=s(B, N + 1, nx), C=s(B, N, mc, nx), h=s(B, N, mc), z=s(B, (nx + ns) * (N + 1) + 2 * nu * N),
                x0=s(B, nx), u_prev=s(B, nu), traj_local=s(B, N + 1, 2), kkt=s(B),
                mdims=L.cmpc_mpc_dims(nx, nu, N, ns, mc, B), w=w, keep=keep, opts=L.opts())


def call_dev(ctx, which, a, null=()):
    from cmpc.solver import _tptr

    P = lambda k: None if k in null else _tptr(a[k])         # noqa: E731
    R = lambda k: None if k in null else ct.byref(a[k])      # noqa: E731
    tab = L.cmpc_lin_table(P("tA"), P("tB"), P("tq"), P("tC"), P("th"))
    tab = None if "table" in null else ct.byref(tab)
    lib = ctx.lib
    if which == "build":
        return lib.cmpc_lin_table_build_dev(ctx.h, R("prm"), R("dims"), a["nu"], R("tdims"), tab, a["t"], P("nbr"),
                                            P("traj_all"), P("A"), P("B"), P("qlin"), P("C"), P("h"), None)
    data = L.cmpc_mpc_data(P("A"), P("B"), P("x0"), P("u_prev"), P("qlin"), P("C"), P("h"))
    out = L.cmpc_mpc_out(P("z"), P("kkt"), None, None)
    return lib.cmpc_lin_table_round_dev(ctx.h, R("prm"), R("dims"), P("nbr"), R("tdims"), tab, a["t"], P("traj_all"),
                                        R("mdims"), R("w"), None if "data" in null else ct.byref(data),
                                        None if "out" in null else ct.byref(out), R("opts"), P("traj_local"), None)


def refused(ctx, which, a, what, null=()):
    import torch

    assert call_dev(ctx, which, a, null) == L.CMPC_ERR_ARG, (which, what)
    assert ctx.lib.cmpc_last_error(ctx.h)
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert bool((a[k] == SENTINEL).all()), (which, what, k)


def test_device_entry_argument_errors(gpu_ctx):
    import torch

    INT_MAX = 2 ** 31 - 1
    bad = [dict(prm=dict(ix=1, iy=1)), dict(prm=dict(ix=-1)), dict(prm=dict(ix=4)), dict(prm=dict(iy=-1)),
           dict(prm=dict(iy=4)), dict(dims=dict(nb=-1)), dict(dims=dict(mo=-1)), dict(dims=dict(mo=4, nb=13)),
           dict(dims=dict(nx=0)), dict(dims=dict(nx=13)), dict(dims=dict(N=0)), dict(dims=dict(batch=-1)),
           dict(dims=dict(self_offset=-1)), dict(tdims=dict(T=0)), dict(tdims=dict(T=-3)), dict(tdims=dict(mode=2)),
           dict(tdims=dict(mode=-1))]
    nulls = dict(build=("prm", "dims", "tdims", "table", "tA", "tB", "tq", "tC", "th", "nbr", "traj_all", "A", "B", "qlin",
                        "C", "h"),
                 round=("prm", "dims", "tdims", "table", "tA", "tB", "tq", "tC", "th", "nbr", "traj_all", "mdims", "w",
                        "data", "out", "z", "A", "B", "x0", "u_prev", "qlin", "C", "h", "traj_local"))
    for which in ("build", "round"):
        for kw in bad:
            a = dev_args(**kw)
            if which == "round":                            # keep the two dims structs in step: the rule under test
                a["mdims"] = L.cmpc_mpc_dims(a["dims"].nx, 2, a["dims"].N, 3, a["dims"].mo + a["dims"].nb, a["dims"].batch)
            refused(gpu_ctx, which, a, kw)
        for k in nulls[which]:
            refused(gpu_ctx, which, dev_args(), k, null=(k,))
        for t in (-1, INT_MAX - 2, INT_MAX):                # t > INT_MAX - N with N = 3
            refused(gpu_ctx, which, dict(dev_args(), t=t), t)
    for nu in (0, 5, -1):
        refused(gpu_ctx, "build", dict(dev_args(), nu=nu), nu)
        a = dev_args()
        a["mdims"] = L.cmpc_mpc_dims(4, nu, 3, 3, 6, 2)
        refused(gpu_ctx, "round", a, nu)
    # the round: mpc_dims must describe the same agents
    for md in ((5, 2, 3, 3, 6, 2), (4, 2, 4, 3, 6, 2), (4, 2, 3, 3, 6, 3), (4, 2, 3, 3, 5, 2), (4, 2, 3, 3, 7, 2)):
        a = dev_args()
        a["mdims"] = L.cmpc_mpc_dims(*md)
        refused(gpu_ctx, "round", a, md)
    # the solver's own rules, before the first launch: CMPC_FLAG_LPV_AUTO on a device entry, an unknown flag
    for flags in (L.CMPC_FLAG_LPV_AUTO, 1 << 20):
        a = dev_args()
        a["opts"] = L.opts(flags=flags)
        refused(gpu_ctx, "round", a, flags)
    # the largest time is taken; mo == 0 / nb == 0: the optional pointers may be NULL
    a = dict(dev_args(), t=INT_MAX - 3)
    assert call_dev(gpu_ctx, "build", a) == L.CMPC_OK
    a = dev_args(dims=dict(mo=0, nb=2))
    a["C"], a["h"] = a["C"][:, :, :2].contiguous(), a["h"][:, :, :2].contiguous()
    assert call_dev(gpu_ctx, "build", a, null=("tC", "th")) == L.CMPC_OK
    a = dev_args(dims=dict(nb=0))
    assert call_dev(gpu_ctx, "build", a, null=("nbr",)) == L.CMPC_OK
    torch.cuda.synchronize()
    assert bool((a["A"] == 0.0).all()) and bool((a["qlin"] == 0.0).all())    # the launch ran: the zero table's window
    # batch == 0: CMPC_OK without a launch
    for which in ("build", "round"):
        a = dev_args(dims=dict(batch=0))
        a["mdims"] = L.cmpc_mpc_dims(4, 2, 3, 3, 6, 0)
        assert call_dev(gpu_ctx, which, a) == L.CMPC_OK, which
        torch.cuda.synchronize()
        for k in OUTPUTS:
            assert bool((a[k] == SENTINEL).all()), (which, k)


def raw_create(ctx, m, mode=HOLD, t0=0, T=None, dims=None, prm=None, init=None, flags=0, null=()):
    """cmpc_lin_rounds_create_table on model `m` with fields replaced; returns (rc, handle)."""
    from cmpc.solver import _weights

    sh, n, tb = m["shared"], m["x0"].shape[0], m["table"]
    d = dict(n_total=n, batch=n, self_offset=0, N=sh["N"], nb=m["nbr"].shape[1], flags=0, history=1, nx=sh["nx"],
             nu=sh["nu"], ns=sh["ns"], mo=sh["mc"] - m["nbr"].shape[1])
    d.update(dims or {})
    cd = L.cmpc_lin_rounds_dims(*[d[k] for k in ("n_total", "batch", "self_offset", "N", "nb", "flags", "history", "nx",
                                                 "nu", "ns", "mo")])
    p = dict(m["prm"])
    p.update(prm or {})
    cp = L.cmpc_lin_params(p["ix"], p["iy"], p["min_dist"], p["wq"])
    w, keep = _weights(sh)
    a = dict(A=L.f64(tb["A"]), B=L.f64(tb["B"]), qlin=L.f64(tb["qlin"]), C=L.f64(tb["C"]), h=L.f64(tb["h"]),
             x0=L.f64(m["x0"]), u_prev=L.f64(m["u_prev"]), nbr=L.i32(m["nbr"]), traj=L.f64(m["traj"]))
    a.update(init or {})
    order = ("A", "B", "qlin", "C", "h", "x0", "u_prev", "nbr", "traj")
    ci = L.cmpc_lin_rounds_table_init(m["T"] if T is None else T, mode, t0,
                                      *[None if k in null else (L.iptr(a[k]) if k == "nbr" else L.dptr(a[k])) for k in order])
    co = L.opts(flags=flags)
    h = ct.c_void_p()
    ref = lambda name, v: None if name in null else ct.byref(v)  # noqa: E731
    rc = ctx.lib.cmpc_lin_rounds_create_table(ctx.h, ref("prm", cp), ref("w", w), ref("dims", cd), ref("init", ci),
                                              ref("opts", co), None if "out" in null else ct.byref(h))
    return rc, h


def test_create_and_handle_argument_errors(gpu_ctx, ltv14):
    from cmpc import CmpcError
    from cmpc.rounds import LinRoundsHandle

    m, lib = ltv14, gpu_ctx.lib
    for kw in (dict(null=("opts",)), dict(mode=PERIODIC, t0=13), dict(dims=dict(flags=L.CMPC_ROUNDS_NO_HALT, history=0)),
               dict(dims=dict(batch=6, self_offset=6, flags=L.CMPC_ROUNDS_HOST_EXCHANGE))):
        rc, h = raw_create(gpu_ctx, m, **kw)
        assert rc == L.CMPC_OK and h.value, kw
        t = ct.c_int(-1)
        assert lib.cmpc_lin_rounds_get_time(h, ct.byref(t)) == L.CMPC_OK and t.value == kw.get("t0", 0)
        assert lib.cmpc_lin_rounds_get_time(h, None) == L.CMPC_ERR_ARG
        assert lib.cmpc_lin_rounds_destroy(h) == L.CMPC_OK
    far, neg = m["nbr"].copy(), m["nbr"].copy()
    far[4, 1], neg[0, 0] = 12, -1
    bad = [dict(null=(k,)) for k in ("prm", "w", "dims", "init", "out", "A", "B", "qlin", "C", "h", "x0", "u_prev", "nbr",
                                     "traj")] + \
          [dict(T=0), dict(T=-1), dict(mode=2), dict(mode=-1), dict(t0=-1), dict(t0=14), dict(t0=15, mode=PERIODIC),
           dict(dims=dict(batch=0)), dict(dims=dict(batch=13)), dict(dims=dict(self_offset=-1)),
           dict(dims=dict(batch=6, self_offset=8, flags=L.CMPC_ROUNDS_HOST_EXCHANGE)), dict(dims=dict(N=0)),
           dict(dims=dict(nb=-1)), dict(dims=dict(mo=-1)), dict(dims=dict(mo=15)), dict(dims=dict(nx=0)),
           dict(dims=dict(nx=13)), dict(dims=dict(nu=0)), dict(dims=dict(nu=5)), dict(dims=dict(ns=-1)),
           dict(dims=dict(ns=5)), dict(prm=dict(ix=8)), dict(prm=dict(ix=9)), dict(prm=dict(iy=-1)),
           dict(init=dict(nbr=far)), dict(init=dict(nbr=neg)), dict(dims=dict(batch=6)),
           dict(dims=dict(history=-1)), dict(dims=dict(flags=16)), dict(dims=dict(flags=-1)),
           dict(dims=dict(nb=12, mo=4, flags=L.CMPC_ROUNDS_RESELECT)), dict(flags=1 << 20)]
    for kw in bad:
        rc, h = raw_create(gpu_ctx, m, **kw)
        assert rc == L.CMPC_ERR_ARG and not h.value, kw
        assert lib.cmpc_last_error(gpu_ctx.h)
    for fn, args in ((lib.cmpc_lin_rounds_get_time, (None, None)), (lib.cmpc_lin_rounds_set_time, (None, 0)),
                     (lib.cmpc_lin_rounds_table_write, (None, 0, 0, None))):
        assert fn(*args) == L.CMPC_ERR_ARG
    # table_write: the row range, no wrap; a refused write leaves the table as it was
    H = table_handle(m, gpu_ctx, PERIODIC)
    rows = {k: v[:, :3] for k, v in m["table"].items()}
    zeros = {k: np.zeros_like(v) for k, v in rows.items()}
    for first in (12, 14, -1):
        with pytest.raises(CmpcError) as e:
            H.write_table(first, **zeros)                    # first_row + count > T, or first_row < 0
        assert e.value.code == L.CMPC_ERR_ARG
    assert H._fn == "cmpc_lin_rounds_" and lib.cmpc_lin_rounds_table_write(H.h, 0, 1, None) == L.CMPC_ERR_ARG
    empty = L.cmpc_lin_table(None, None, None, None, None)
    assert lib.cmpc_lin_rounds_table_write(H.h, 0, -1, ct.byref(empty)) == L.CMPC_ERR_ARG
    assert lib.cmpc_lin_rounds_table_write(H.h, 14, 0, ct.byref(empty)) == L.CMPC_OK       # nothing, at the end
    H.write_table(11, **rows)                                # rows 11..13: the last that fit
    H.write_table(11, **{k: v[:, 11:] for k, v in m["table"].items()})       # and back
    want = host_round(m, gpu_ctx, PERIODIC, 0, m["x0"], m["u_prev"], m["traj"])
    assert H.step() == 1
    assert_bytes(handle_state(H), want, "after the refused writes")
    H.close()
    # a fixed-window handle has no time to set and no table to write
    A0, B0, own0 = S.lin_window(m["table"], 0, m["shared"]["N"], HOLD)
    F = LinRoundsHandle(m["shared"], m["prm"], own0, A0, B0, m["x0"], m["u_prev"], m["nbr"], m["traj"], ctx=gpu_ctx)
    t = ct.c_int(-1)
    assert lib.cmpc_lin_rounds_get_time(F.h, ct.byref(t)) == L.CMPC_OK and t.value == 0
    assert lib.cmpc_lin_rounds_set_time(F.h, 0) == L.CMPC_ERR_ARG
    one = {k: L.f64(v[:, :1]) for k, v in m["table"].items()}
    tab = L.cmpc_lin_table(*[L.dptr(one[k]) for k in ("A", "B", "qlin", "C", "h")])
    assert lib.cmpc_lin_rounds_table_write(F.h, 0, 1, ct.byref(tab)) == L.CMPC_ERR_ARG
    assert F.step() == 1
    assert_bytes(handle_state(F), want, "the fixed window at t = 0")
    assert lib.cmpc_lin_rounds_get_time(F.h, ct.byref(t)) == L.CMPC_OK and t.value == 0
    F.close()
    # the handle does not duplicate the solver's rules: CMPC_FLAG_LPV_AUTO passes create and fails the first step,
    # and a round that did not run does not move the time
    rc, h = raw_create(gpu_ctx, m, flags=L.CMPC_FLAG_LPV_AUTO, t0=3)
    assert rc == L.CMPC_OK
    done = ct.c_int(-1)
    assert lib.cmpc_lin_rounds_step(h, 2, ct.byref(done)) == L.CMPC_ERR_ARG and done.value == 0
    assert lib.cmpc_lin_rounds_get_time(h, ct.byref(t)) == L.CMPC_OK and t.value == 3
    assert lib.cmpc_lin_rounds_destroy(h) == L.CMPC_OK
