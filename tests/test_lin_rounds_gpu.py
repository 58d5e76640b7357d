"""The linear-model round family on the device (cmpc_lin_build_dev / _advance_dev / _round_dev, cmpc_lin_rounds_*):
the builder kernel against its numpy statement, the double integrator as a special case against the trusted
double-integrator chain (bit for bit), a 9-state time-varying model neither other family covers against a host
loop, and the handle's behaviour and argument errors."""
import ctypes as ct

import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S

pytestmark = pytest.mark.gpu


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


# ---- 1. the builder kernel against lin_rows ----

# (nx, mo, nb, N, batch, ix, iy): the double integrator's shape; position columns away from 0, 1; iy < ix and no
# own rows; no neighbours (the copies alone); more stages than the workgroup has lanes
BUILD_SHAPES = [(4, 4, 2, 3, 5, 0, 1), (9, 4, 3, 2, 3, 7, 8), (12, 0, 1, 1, 1, 11, 0), (6, 2, 0, 4, 2, 0, 1),
                (4, 4, 2, 70, 2, 0, 1)]


def build_instance(shape, seed):
    nx, mo, nb, N, B, ix, iy = shape
    rng = np.random.default_rng(seed)
    n, off = B + 3, 1                                   # local agents: rows 1 .. B of the exchange buffer
    own = dict(qlin_own=rng.standard_normal((B, N + 1, nx)), C_own=rng.standard_normal((B, N, mo, nx)),
               h_own=rng.standard_normal((B, N, mo)))
    traj = rng.standard_normal((n, N + 1, 2))
    nbr = np.zeros((B, nb), np.int32)
    for b in range(B):
        nbr[b] = rng.permutation([j for j in range(n) if j != off + b])[:nb]
    return dict(ix=ix, iy=iy, min_dist=0.25, wq=5.0), own, nbr, traj, off


def run_build(gpu_ctx, prm, own, nbr, traj, off):
    import torch
    from cmpc.rounds import lin_build_dev

    mo = own["C_own"].shape[2]
    d_own = dict(qlin_own=dev(own["qlin_own"]), C_own=dev(own["C_own"]) if mo else None,
                 h_own=dev(own["h_own"]) if mo else None)
    out = lin_build_dev(prm, d_own, dev(nbr) if nbr.shape[1] else None, dev(traj), off, ctx=gpu_ctx)
    torch.cuda.synchronize()
    return [host(t) for t in out]


@pytest.mark.parametrize("shape", BUILD_SHAPES)
def test_builder_kernel_equals_lin_rows(gpu_ctx, shape):
    prm, own, nbr, traj, off = build_instance(shape, 11)
    nx, mo, nb, N, B, ix, iy = shape
    if shape == BUILD_SHAPES[0]:                        # negative zeros in the own arrays survive the copies
        own["qlin_own"][:, ::2] = -0.0
        own["C_own"][:, :, 1] = -0.0
        own["h_own"][:, 0] = -0.0
    if shape == BUILD_SHAPES[1]:                        # agent 1's neighbour 2 (row 5: no local agent) sits on
        nbr[1] = [0, 3, 5]                              # its point at stage 1
        traj[5, 1] = traj[off + 1, 1]
    want = S.lin_rows(prm, own, nbr, traj, off)
    got = run_build(gpu_ctx, prm, own, nbr, traj, off)
    for name, g, w in zip(("qlin", "C", "h"), got, want):
        assert same(g, w), name
    q, C, h = got
    if shape == BUILD_SHAPES[0]:
        assert np.signbit(C[:, :, 1]).all() and np.signbit(h[:, 0, :mo]).all() and np.signbit(q[:, 0]).all()
    if shape == BUILD_SHAPES[1]:
        assert np.isnan(C[1, 1, mo + 2, [ix, iy]]).all() and np.isnan(h[1, 1, mo + 2]) and np.isnan(q[1, 2, [ix, iy]]).all()
        assert np.isnan(C).sum() == 2 and np.isnan(h).sum() == 1 and np.isnan(q).sum() == 2
    else:
        assert all(np.isfinite(a).all() for a in got)


# ---- 2. the double integrator as a special case ----

@pytest.mark.parametrize("dim", [2, 3])
def test_builder_of_the_double_integrator_equals_di_build(gpu_ctx, dim):
    import torch
    from cmpc.rounds import DIRounds

    sc = S.make_di(16, 6, 2, dim)
    R = DIRounds(sc, ctx=gpu_ctx, fused=False)
    R.build()
    torch.cuda.synchronize()
    lin = S.lin_of_di(sc)
    got = run_build(gpu_ctx, lin["prm"], lin["own"], lin["nbr"], lin["traj"], lin["self_offset"])
    for name, g, t in zip(("qlin", "C", "h"), got, (R.qlin, R.C, R.h)):
        w = host(t)
        assert np.isfinite(w).all() and g.shape == w.shape and g.tobytes() == w.tobytes(), name


# ---- 3. rounds against the trusted chain ----

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
def test_rounds_of_the_double_integrator_equal_the_unfused_chain(gpu_ctx, shape, rounds, lpt):
    """build -> cmpc_solve_mpc_batch_dev -> advance -> exchange (DIRounds, fused=False) against the handle of the
    same scenario in the new family; the second shape runs the stage-wise Riccati solver, with the launch order."""
    import torch
    from cmpc.rounds import DIRounds, LinRoundsHandle

    sc = S.make_di(*shape)
    R = DIRounds(sc, ctx=gpu_ctx, fused=False, lpt=lpt)
    H = LinRoundsHandle.of_di(sc, ctx=gpu_ctx, lpt=lpt)
    for rnd in range(rounds):
        R.step()
        torch.cuda.synchronize()
        want = {k: host(getattr(R, k)) for k in KEYS}
        want["traj"] = host(R.traj_all)                  # the exchange buffer (one rank: every agent's row)
        assert H.step() == 1
        assert_bytes(handle_state(H), want, rnd)
        assert np.isfinite(want["z"]).all() and (want["iters"] > 0).all()
    if lpt:
        assert len(set(want["iters"].tolist())) > 1      # the last launch order was not the identity's
    H.close()


def test_rounds_of_the_double_integrator_equal_the_fused_handle(gpu_ctx):
    """The fused launch (DIRoundsHandle: rows built in the solver's LDS) is held bit-equal to build-then-solve by
    tests/test_gpu.py, so the new family's handle must agree with it too."""
    from cmpc.rounds import DIRoundsHandle, LinRoundsHandle

    sc = S.make_di(64, 10, 2, 2)
    D = DIRoundsHandle(sc, ctx=gpu_ctx, lpt=False)
    H = LinRoundsHandle.of_di(sc, ctx=gpu_ctx, lpt=False)
    for rnd in range(4):
        assert D.step() == 1 and H.step() == 1
        want = D.read()
        want["traj"] = D.get_traj()
        assert_bytes(handle_state(H), want, rnd, KEYS + ("traj", "nbr"))
    D.close()
    H.close()


# ---- 4. a model neither family covers ----

def make_ltv(n=12, N=10, nb=2, seed=7):
    """12 agents on the three-lane road of make_di with a 9-state model, the reference's row / slack pattern and
    its dimensions (9, 2, 3; mc = 4 + nb): x = [v_x, v_y, c2, e_y, c4, c5, c6, X, Y], u = (a_y, a_x); X, Y in
    columns 7, 8; A_k = I + dt (kinematics + seeded perturbation), B_k likewise: time-varying, every agent its own."""
    rng = np.random.default_rng(seed)
    nx, nu, ns, dt = 9, 2, 3, S.DT
    Ac = np.zeros((nx, nx))
    Ac[7, 0] = Ac[8, 1] = Ac[3, 1] = 1.0                # X' = v_x, Y' = v_y, e_y' = v_y
    for c in (2, 4, 5, 6):
        Ac[c, c] = -2.0                                  # the spare states decay
    Bc = np.zeros((nx, nu))
    Bc[0, 1] = Bc[1, 0] = 1.0
    Bc[2, 0] = Bc[4, 1] = 0.1
    A = np.eye(nx) + dt * (Ac + 0.02 * rng.standard_normal((n, N, nx, nx)))
    B = dt * (Bc + 0.02 * rng.standard_normal((n, N, nx, nu)))
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
    C_own = np.zeros((n, N, 4, nx))
    C_own[:, :, 0, 0], C_own[:, :, 1, 0], C_own[:, :, 2, 3], C_own[:, :, 3, 3] = -1.0, 1.0, 1.0, -1.0
    h_own = np.broadcast_to(np.array([-0.0, 5.5, 0.75, 0.75]), (n, N, 4)).copy()
    qlin_own = np.zeros((n, N + 1, nx))
    qlin_own[:, :, 0] = -3.0 * 10.0
    return dict(shared=shared, prm=dict(ix=7, iy=8, min_dist=0.25, wq=5.0),
                own=dict(qlin_own=qlin_own, C_own=C_own, h_own=h_own), A=A, B=B, x0=x0, u_prev=np.zeros((n, nu)),
                nbr=S.nearest_neighbours(x0[:, 7:9], nb), traj=traj)


def ltv_handle(m, ctx, **kw):
    from cmpc.rounds import LinRoundsHandle

    return LinRoundsHandle(m["shared"], m["prm"], m["own"], m["A"], m["B"], m["x0"], m["u_prev"], m["nbr"], m["traj"],
                           ctx=ctx, **kw)


def host_round(m, ctx, x0, u_prev, traj, nbr=None):
    """lin_rows -> cmpc.solve_mpc -> lin_advance: one round on the host's side of the ABI."""
    import cmpc

    sh = m["shared"]
    qlin, C, h = S.lin_rows(m["prm"], m["own"], m["nbr"] if nbr is None else nbr, traj)
    P = dict(sh, A=m["A"], B=m["B"], x0=x0, u_prev=u_prev, qlin=qlin, C=C, h=h)
    z, kkt, iters, status = cmpc.solve_mpc(P, ctx)
    x1, u1, t1 = S.lin_advance(m["prm"], z, sh["nx"], sh["nu"], sh["ns"], sh["N"], x0, u_prev, traj)
    return dict(z=z, kkt=kkt, iters=iters, status=status, x0=x1, u_prev=u1, traj=t1)


@pytest.fixture(scope="module")
def ltv():
    return make_ltv()


def test_rounds_of_a_time_varying_model_equal_the_host_loop(gpu_ctx, ltv):
    m = ltv
    assert not np.array_equal(m["A"][:, 0], m["A"][:, 1])            # time-varying
    H = ltv_handle(m, gpu_ctx)
    x0, up, traj = m["x0"], m["u_prev"], m["traj"]
    for rnd in range(3):
        want = host_round(m, gpu_ctx, x0, up, traj)
        assert (want["status"] == L.CMPC_SOLVED).all(), (rnd, want["status"])    # the comparator alone
        assert H.step() == 1
        assert_bytes(handle_state(H), want, rnd)
        assert not np.array_equal(want["traj"], traj)
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    H.close()


# ---- 5. behaviour ----

def test_advance_kernel_skips_a_non_finite_agent(gpu_ctx):
    import torch
    from cmpc.rounds import lin_advance_dev

    rng = np.random.default_rng(3)
    nx, nu, ns, N, B = 5, 2, 1, 70, 4                    # 2 (N + 1) trajectory entries: more than one pass of lanes
    z = rng.standard_normal((B, (nx + ns) * (N + 1) + 2 * nu * N))
    z[1, -1] = np.nan                                    # the last du entry: never copied, still disqualifies
    z[2, 0] = -np.inf
    x0, up, tr = rng.standard_normal((B, nx)), rng.standard_normal((B, nu)), rng.standard_normal((B, N + 1, 2))
    prm = dict(ix=4, iy=1, min_dist=0.25, wq=5.0)
    want = S.lin_advance(prm, z, nx, nu, ns, N, x0, up, tr)
    d = [dev(a) for a in (x0, up, tr)]
    lin_advance_dev(prm, dev(z), nx, nu, ns, N, *d, ctx=gpu_ctx)
    torch.cuda.synchronize()
    for g, w, before in zip(d, want, (x0, up, tr)):
        assert host(g).tobytes() == w.tobytes()
        assert np.array_equal(w[[1, 2]], before[[1, 2]]) and not np.array_equal(w[[0, 3]], before[[0, 3]])


def test_set_state_and_the_non_finite_guard(gpu_ctx, ltv):
    m = ltv
    H = ltv_handle(m, gpu_ctx)
    assert H.step() == 1
    a = handle_state(H)
    # the measured state replaces the predicted one: the next round solves from it
    x0 = a["x0"].copy()
    x0[:, 0] += 0.05
    up = a["u_prev"] + 0.01
    H.set_state(x0, up)
    b = H.read()
    assert b["x0"].tobytes() == x0.tobytes() and b["u_prev"].tobytes() == up.tobytes()
    want = host_round(m, gpu_ctx, x0, up, a["traj"])
    assert H.step() == 1
    c = handle_state(H)
    assert_bytes(c, want, "set_state")
    # either part may be left alone
    H.set_state(None, up)
    assert H.read()["x0"].tobytes() == c["x0"].tobytes() and H.read()["u_prev"].tobytes() == up.tobytes()
    # an agent with a NaN state keeps its state and its trajectory row; the others advance
    bad = c["x0"].copy()
    bad[5, 0] = np.nan
    H.set_state(bad, c["u_prev"])
    assert H.step() == 1
    e = handle_state(H)
    assert not np.isfinite(e["z"][5]).all()
    assert same(e["x0"][5], bad[5]) and e["u_prev"][5].tobytes() == c["u_prev"][5].tobytes()
    assert e["traj"][5].tobytes() == c["traj"][5].tobytes() and np.isfinite(e["traj"]).all()
    others = [i for i in range(12) if i != 5]
    assert np.isfinite(e["z"][others]).all() and not np.array_equal(e["traj"][others], c["traj"][others])
    with pytest.raises(ValueError):
        H.set_state(bad[:3])
    H.close()


def test_reselect_follows_the_exchange_buffer(gpu_ctx, ltv):
    m = dict(ltv)
    p = m["traj"][:, 0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    m["nbr"] = np.argsort(-d2, axis=1, kind="stable")[:, :2].astype(np.int32)    # the farthest: a valid table
    first = S.select_neighbours(m["traj"], 2)
    assert (m["nbr"] != first).any(axis=1).all()
    H = ltv_handle(m, gpu_ctx, reselect=True)
    x0, up, traj = m["x0"], m["u_prev"], m["traj"]
    for rnd in range(2):
        sel = S.select_neighbours(traj, 2)               # on the buffer as the last exchange left it
        want = host_round(m, gpu_ctx, x0, up, traj, nbr=sel)
        assert H.step() == 1
        got = handle_state(H)
        assert np.array_equal(got["nbr"], sel)
        assert_bytes(got, want, rnd)
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    H.close()


def test_log_rows_and_ring_errors(gpu_ctx, ltv):
    """The log's rows are log_row with look_col = ix; history and log ranges fail where DIRoundsHandle's do."""
    from cmpc import CmpcError
    from cmpc.rounds import DIRoundsHandle

    m, sh = ltv, ltv["shared"]
    H = ltv_handle(m, gpu_ctx, history=2, log=2)
    D = DIRoundsHandle(S.make_di(6, 9, 2, 2), ctx=gpu_ctx, history=2, log=2)
    zs = []
    for rnd in range(3):
        assert H.step() == 1 and D.step() == 1
        zs.append(H.read())
    assert H.log_range() == D.log_range() == (1, 2)
    lg = H.log()
    for i, rnd in enumerate((1, 2)):
        state, u, look = S.log_row(zs[rnd]["z"], sh["nx"], sh["nu"], sh["ns"], sh["N"], m["prm"]["ix"])
        assert lg["state"][i].tobytes() == state.tobytes() and lg["u"][i].tobytes() == u.tobytes()
        assert lg["look_ahead"][i].tobytes() == look.tobytes() and (look > 0).all()     # the advance along X
        for k in ("kkt", "iters", "status"):
            assert lg[k][i].tobytes() == zs[rnd][k].tobytes(), (rnd, k)
    hist = H.history(1, 2)
    for i, rnd in enumerate((1, 2)):
        for k in ("kkt", "iters", "status"):
            assert hist[k][i].tobytes() == zs[rnd][k].tobytes(), (rnd, k)

    def outcome(fn, *args):
        try:
            fn(*args)
            return L.CMPC_OK
        except CmpcError as e:
            return e.code

    for first, count in ((0, 1), (0, 3), (1, 2), (2, 1), (2, 2), (3, 0), (3, 1), (-1, 1), (1, -1)):
        assert outcome(H.history, first, count) == outcome(D.history, first, count), (first, count)
        assert outcome(H.log, first, count) == outcome(D.log, first, count), (first, count)
    assert outcome(H.history, 0, 1) == L.CMPC_ERR_ARG and outcome(H.log, 3, 1) == L.CMPC_ERR_ARG
    assert outcome(H._call, "log_enable", 2, 0) == L.CMPC_ERR_ARG          # twice
    H.close()
    D.close()


# ---- the argument errors of the three device entry points ----

def dev_args(ctx, prm=None, dims=None):
    """Valid device arguments of cmpc_lin_build_dev / _advance_dev / _round_dev on a (4, 2, 3) model, fields
    replaced; a call that passes its checks would launch on them."""
    import torch
    from cmpc.solver import _weights

    p = dict(ix=0, iy=1, min_dist=0.25, wq=5.0)
    p.update(prm or {})
    d = dict(batch=2, N=3, nb=2, self_offset=0, nx=4, mo=4)
    d.update(dims or {})
    B, N, nx, nu, ns, mc = 2, 3, 4, 2, 3, 6
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    sh = dict(S.di_shared(2, N, 2))
    w, keep = _weights(sh)
    a = dict(prm=L.cmpc_lin_params(p["ix"], p["iy"], p["min_dist"], p["wq"]),
             dims=L.cmpc_lin_dims(*[d[k] for k in ("batch", "N", "nb", "self_offset", "nx", "mo")]),
             nbr=torch.ones((B, 2), dtype=torch.int32, device="cuda"), qlin_own=t(B, N + 1, nx), C_own=t(B, N, 4, nx),
             h_own=t(B, N, 4), traj_all=t(4, N + 1, 2), qlin=t(B, N + 1, nx), C=t(B, N, mc, nx), h=t(B, N, mc),
             z=t(B, (nx + ns) * (N + 1) + 2 * nu * N), x0=t(B, nx), u_prev=t(B, nu), traj_local=t(B, N + 1, 2),
             A=t(B, N, nx, nx), B=t(B, N, nx, nu), kkt=t(B), mdims=L.cmpc_mpc_dims(nx, nu, N, ns, mc, B), w=w, keep=keep,
             opts=L.opts())
    return a


def call_dev(ctx, which, a, null=()):
    from cmpc.solver import _tptr

    P = lambda k: None if k in null else _tptr(a[k])         # noqa: E731
    R = lambda k: None if k in null else ct.byref(a[k])      # noqa: E731
    own = L.cmpc_lin_own(P("qlin_own"), P("C_own"), P("h_own"))
    own = None if "own" in null else ct.byref(own)
    lib = ctx.lib
    if which == "build":
        return lib.cmpc_lin_build_dev(ctx.h, R("prm"), R("dims"), P("nbr"), own, P("traj_all"), P("qlin"), P("C"),
                                      P("h"), None)
    if which == "advance":
        return lib.cmpc_lin_advance_dev(ctx.h, R("prm"), R("dims"), a.get("ns", 3), a.get("nu", 2), P("z"), P("x0"),
                                        P("u_prev"), P("traj_local"), None)
    data = L.cmpc_mpc_data(P("A"), P("B"), P("x0"), P("u_prev"), P("qlin"), P("C"), P("h"))
    out = L.cmpc_mpc_out(P("z"), P("kkt"), None, None)
    return lib.cmpc_lin_round_dev(ctx.h, R("prm"), R("dims"), P("nbr"), own, P("traj_all"), R("mdims"), R("w"),
                                  None if "data" in null else ct.byref(data), None if "out" in null else ct.byref(out),
                                  R("opts"), P("traj_local"), None)


def test_device_entry_argument_errors(gpu_ctx):
    import torch

    bad_dims = [dict(prm=dict(ix=1, iy=1)), dict(prm=dict(ix=-1)), dict(prm=dict(ix=4)), dict(prm=dict(iy=-1)),
                dict(prm=dict(iy=4)), dict(dims=dict(nb=-1)), dict(dims=dict(mo=-1)), dict(dims=dict(mo=4, nb=13)),
                dict(dims=dict(nx=0)), dict(dims=dict(nx=13)), dict(dims=dict(N=0)), dict(dims=dict(batch=-1)),
                dict(dims=dict(self_offset=-1))]
    nulls = dict(build=("prm", "dims", "own", "qlin_own", "C_own", "h_own", "nbr", "traj_all", "qlin", "C", "h"),
                 advance=("prm", "dims", "z", "x0", "u_prev", "traj_local"),
                 round=("prm", "dims", "own", "qlin_own", "C_own", "h_own", "nbr", "traj_all", "mdims", "w", "data", "out",
                        "z", "x0", "u_prev", "qlin", "C", "h", "traj_local"))
    for which in ("build", "advance", "round"):
        for kw in bad_dims:
            a = dev_args(gpu_ctx, **kw)
            if which == "round":                            # keep the two dims structs in step: the rule under test
                a["mdims"] = L.cmpc_mpc_dims(a["dims"].nx, 2, a["dims"].N, 3, a["dims"].mo + a["dims"].nb, a["dims"].batch)
            assert call_dev(gpu_ctx, which, a) == L.CMPC_ERR_ARG, (which, kw)
            assert gpu_ctx.lib.cmpc_last_error(gpu_ctx.h)
        for k in nulls[which]:
            assert call_dev(gpu_ctx, which, dev_args(gpu_ctx), null=(k,)) == L.CMPC_ERR_ARG, (which, k)
    for ns, nu in ((-1, 2), (5, 2), (3, 0), (3, 5)):
        assert call_dev(gpu_ctx, "advance", dict(dev_args(gpu_ctx), ns=ns, nu=nu)) == L.CMPC_ERR_ARG
    # the round: mpc_dims must describe the same agents
    for md in ((5, 2, 3, 3, 6, 2), (4, 2, 4, 3, 6, 2), (4, 2, 3, 3, 6, 3), (4, 2, 3, 3, 5, 2), (4, 2, 3, 3, 7, 2)):
        a = dev_args(gpu_ctx)
        a["mdims"] = L.cmpc_mpc_dims(*md)
        assert call_dev(gpu_ctx, "round", a) == L.CMPC_ERR_ARG, md
    # the solver's own rules come back unchanged: CMPC_FLAG_LPV_AUTO on a device entry, an unknown flag
    for flags in (L.CMPC_FLAG_LPV_AUTO, 1 << 20):
        a = dev_args(gpu_ctx)
        a["opts"] = L.opts(flags=flags)
        assert call_dev(gpu_ctx, "round", a) == L.CMPC_ERR_ARG, flags
    # mo == 0 / nb == 0: the optional pointers may be NULL; batch == 0: CMPC_OK without a launch
    a = dev_args(gpu_ctx, dims=dict(mo=0, nb=2))
    a["C"], a["h"] = a["C"][:, :, :2].contiguous(), a["h"][:, :, :2].contiguous()
    a["traj_all"][:] = torch.arange(4, device="cuda", dtype=torch.float64)[:, None, None]
    assert call_dev(gpu_ctx, "build", a, null=("C_own", "h_own")) == L.CMPC_OK
    a = dev_args(gpu_ctx, dims=dict(nb=0))
    assert call_dev(gpu_ctx, "build", a, null=("nbr",)) == L.CMPC_OK
    for which in ("build", "advance", "round"):
        a = dev_args(gpu_ctx, dims=dict(batch=0))
        a["mdims"] = L.cmpc_mpc_dims(4, 2, 3, 3, 6, 0)
        a["qlin"][:] = 7.0
        a["x0"][:] = 7.0
        assert call_dev(gpu_ctx, which, a) == L.CMPC_OK, which
        torch.cuda.synchronize()
        assert (a["qlin"] == 7.0).all() and (a["x0"] == 7.0).all()
    torch.cuda.synchronize()


def raw_create(ctx, m, dims=None, prm=None, init=None, flags=0, null=()):
    """cmpc_lin_rounds_create on model `m` with fields replaced; returns (rc, handle)."""
    from cmpc.solver import _weights

    sh, n = m["shared"], m["x0"].shape[0]
    d = dict(n_total=n, batch=n, self_offset=0, N=sh["N"], nb=m["nbr"].shape[1], flags=0, history=1, nx=sh["nx"],
             nu=sh["nu"], ns=sh["ns"], mo=sh["mc"] - m["nbr"].shape[1])
    d.update(dims or {})
    cd = L.cmpc_lin_rounds_dims(*[d[k] for k in ("n_total", "batch", "self_offset", "N", "nb", "flags", "history", "nx",
                                                 "nu", "ns", "mo")])
    p = dict(m["prm"])
    p.update(prm or {})
    cp = L.cmpc_lin_params(p["ix"], p["iy"], p["min_dist"], p["wq"])
    w, keep = _weights(sh)
    a = dict(A=L.f64(m["A"]), B=L.f64(m["B"]), x0=L.f64(m["x0"]), u_prev=L.f64(m["u_prev"]),
             qlin_own=L.f64(m["own"]["qlin_own"]), C_own=L.f64(m["own"]["C_own"]), h_own=L.f64(m["own"]["h_own"]),
             nbr=L.i32(m["nbr"]), traj=L.f64(m["traj"]))
    a.update(init or {})
    order = ("A", "B", "x0", "u_prev", "qlin_own", "C_own", "h_own", "nbr", "traj")
    ci = L.cmpc_lin_rounds_init(*[None if k in null else (L.iptr(a[k]) if k == "nbr" else L.dptr(a[k])) for k in order])
    co = L.opts(flags=flags)
    h = ct.c_void_p()
    ref = lambda name, v: None if name in null else ct.byref(v)  # noqa: E731
    rc = ctx.lib.cmpc_lin_rounds_create(ctx.h, ref("prm", cp), ref("w", w), ref("dims", cd), ref("init", ci),
                                        ref("opts", co), None if "out" in null else ct.byref(h))
    return rc, h


def test_create_argument_errors(gpu_ctx, ltv):
    m, lib = ltv, gpu_ctx.lib
    for kw in (dict(null=("opts",)), dict(dims=dict(flags=L.CMPC_ROUNDS_NO_HALT, history=0)),
               dict(dims=dict(batch=6, self_offset=6, flags=L.CMPC_ROUNDS_HOST_EXCHANGE))):
        rc, h = raw_create(gpu_ctx, m, **kw)
        assert rc == L.CMPC_OK and h.value, kw
        assert lib.cmpc_lin_rounds_destroy(h) == L.CMPC_OK
    far, neg = m["nbr"].copy(), m["nbr"].copy()
    far[4, 1], neg[0, 0] = 12, -1
    bad = [dict(null=(k,)) for k in ("prm", "w", "dims", "init", "out", "A", "B", "x0", "u_prev", "qlin_own", "C_own",
                                     "h_own", "nbr", "traj")] + \
          [dict(dims=dict(batch=0)), dict(dims=dict(batch=13)), dict(dims=dict(self_offset=-1)),
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
    for fn, args in ((lib.cmpc_lin_rounds_step, (None, 1, None)), (lib.cmpc_lin_rounds_read, (None, None)),
                     (lib.cmpc_lin_rounds_history, (None, 0, 0, None, None, None)),
                     (lib.cmpc_lin_rounds_get_traj, (None, None)), (lib.cmpc_lin_rounds_set_traj, (None, None)),
                     (lib.cmpc_lin_rounds_set_state, (None, None, None)), (lib.cmpc_lin_rounds_log_enable, (None, 1, 0)),
                     (lib.cmpc_lin_rounds_log_range, (None, None, None)),
                     (lib.cmpc_lin_rounds_log_read, (None, 0, 0, None))):
        assert fn(*args) == L.CMPC_ERR_ARG
    assert lib.cmpc_lin_rounds_destroy(None) == L.CMPC_OK
    # the handle does not duplicate the solver's rules: CMPC_FLAG_LPV_AUTO passes create and fails the first step
    rc, h = raw_create(gpu_ctx, m, flags=L.CMPC_FLAG_LPV_AUTO)
    assert rc == L.CMPC_OK
    done = ct.c_int(-1)
    assert lib.cmpc_lin_rounds_step(h, 2, ct.byref(done)) == L.CMPC_ERR_ARG and done.value == 0
    assert lib.cmpc_lin_rounds_destroy(h) == L.CMPC_OK
