"""Consensus steps of the linear-model family on the device (cmpc_lin_publish_dev, cmpc_lin_rounds_step_consensus /
_consensus_read): the publish kernel against its numpy statement, a one-round consensus step against a plain round,
consensus steps against a host loop of the same pieces (fixed window and stage table), the handle's behaviour around
a step, the argument errors and an agent without a finite solution."""
import ctypes as ct

import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S
from lin_consensus_cases import ATOL_T, PUBLISH_SHAPES, make_ltv_table, publish_instance, threshold_instance

pytestmark = pytest.mark.gpu

PERIODIC = L.CMPC_TABLE_PERIODIC
DEFAULTS = dict(min_rounds=3, need=2, max_rounds=12, atol=0.01, rtol=1e-5)
CAPPED = dict(min_rounds=1, need=1, max_rounds=3, atol=1e-7, rtol=0.0)


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


# ---- 1. the publish kernel against lin_publish ----

SENTINEL = 7.0


def run_publish(ctx, shape, inst, atol, rtol, skip=()):
    """cmpc_lin_publish_dev on sentinel-filled outputs (the count zeroed, as the library does); `skip`: outputs
    passed as NULL.  Returns dict(traj_local, close, delta, not_close) of host arrays (None where skipped)."""
    import torch
    from cmpc.rounds import lin_publish_dev

    nx, ns, nu, N, B = shape[:5]
    prm, z, traj, off = inst
    out = dict(close=torch.full((B,), -5, dtype=torch.int32, device="cuda"),
               delta=torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda"),
               not_close=torch.zeros(1, dtype=torch.int32, device="cuda"))
    tl = torch.full((B, N + 1, 2), SENTINEL, dtype=torch.float64, device="cuda")
    lin_publish_dev(prm, dev(z), nx, nu, ns, N, dev(traj), tl, atol=atol, rtol=rtol, self_offset=off, ctx=ctx,
                    **{k: None if k in skip else v for k, v in out.items()})
    torch.cuda.synchronize()
    for k in skip:                                           # a skipped output's buffer was never handed over
        assert bool((out[k] == (0 if k == "not_close" else -5 if k == "close" else SENTINEL)).all())
    return dict(traj_local=host(tl), **{k: None if k in skip else host(v) for k, v in out.items()})


@pytest.mark.parametrize("mode", ["random", "threshold"])
@pytest.mark.parametrize("shape", PUBLISH_SHAPES)
def test_publish_kernel_equals_lin_publish(gpu_ctx, shape, mode):
    nx, ns, nu, N, B = shape[:5]
    inst, atol, rtol = (publish_instance(shape), 0.01, 1e-5) if mode == "random" else (threshold_instance(shape), ATOL_T, 0.0)
    prm, z, traj, off = inst
    tl, close, delta, count = S.lin_publish(prm, z, nx, nu, ns, N, traj, atol=atol, rtol=rtol, self_offset=off)
    got = run_publish(gpu_ctx, shape, inst, atol, rtol)
    assert got["traj_local"].tobytes() == tl.tobytes()          # copies on both sides: NaN payloads included
    assert got["close"].dtype == np.int32 and np.array_equal(got["close"], close)
    assert same(got["delta"], delta)
    assert got["not_close"].tolist() == [count]
    if B > 1:
        assert 0 < count < B                                    # both verdicts occur
    if mode == "random" and B >= 3:
        assert np.isnan(got["delta"][:2]).all() and not got["close"][:2].any()
    # each optional output alone as NULL: the others are what they were
    for skip in ("close", "delta", "not_close"):
        part = run_publish(gpu_ctx, shape, inst, atol, rtol, skip=(skip,))
        for k in ("traj_local", "close", "delta", "not_close"):
            if k != skip:
                assert same(part[k], got[k]) if k == "delta" else part[k].tobytes() == got[k].tobytes(), (skip, k)


def test_publish_argument_errors(gpu_ctx):
    import torch
    from cmpc.solver import _tptr

    nx, ns, nu, N, B, n = 4, 3, 2, 3, 2, 4
    z = torch.zeros((B, (nx + ns) * (N + 1) + 2 * nu * N), dtype=torch.float64, device="cuda")
    traj = torch.zeros((n, N + 1, 2), dtype=torch.float64, device="cuda")
    tl = torch.full((B, N + 1, 2), SENTINEL, dtype=torch.float64, device="cuda")
    close = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    delta = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
    cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")

    def call(prm=(0, 1), dims=None, ns_=ns, nu_=nu, atol=0.01, rtol=1e-5, null=()):
        d = dict(batch=B, N=N, nb=0, self_offset=1, nx=nx, mo=0)
        d.update(dims or {})
        cp = L.cmpc_lin_params(prm[0], prm[1], 0.25, 5.0)
        cd = L.cmpc_lin_dims(*[d[k] for k in ("batch", "N", "nb", "self_offset", "nx", "mo")])
        P = lambda k, t: None if k in null else _tptr(t)          # noqa: E731
        return gpu_ctx.lib.cmpc_lin_publish_dev(gpu_ctx.h, None if "prm" in null else ct.byref(cp),
                                                None if "dims" in null else ct.byref(cd), ns_, nu_, P("z", z),
                                                P("traj_all", traj), atol, rtol, P("traj_local", tl), _tptr(close),
                                                _tptr(delta), _tptr(cnt), None)

    bad = [dict(prm=(1, 1)), dict(prm=(-1, 1)), dict(prm=(0, 4)), dict(dims=dict(nx=0)), dict(dims=dict(nx=13)),
           dict(dims=dict(N=0)), dict(dims=dict(batch=-1)), dict(dims=dict(self_offset=-1)), dict(dims=dict(nb=-1)),
           dict(dims=dict(mo=-1)), dict(ns_=-1), dict(ns_=5), dict(nu_=0), dict(nu_=5), dict(atol=-1e-300),
           dict(atol=float("nan")), dict(rtol=-1.0), dict(rtol=float("nan")), dict(atol=float("-inf"))] + \
          [dict(null=(k,)) for k in ("prm", "dims", "z", "traj_all", "traj_local")]
    for kw in bad:
        assert call(**kw) == L.CMPC_ERR_ARG, kw
        assert gpu_ctx.lib.cmpc_last_error(gpu_ctx.h)
    assert call(dims=dict(batch=0)) == L.CMPC_OK                 # no launch
    torch.cuda.synchronize()
    assert bool((tl == SENTINEL).all()) and bool((close == -5).all()) and bool((delta == SENTINEL).all())
    assert int(cnt.item()) == -5
    assert call(atol=float("inf"), rtol=float("inf")) == L.CMPC_OK    # +inf is allowed; the count is added to
    torch.cuda.synchronize()
    assert bool((tl == 0.0).all()) and int(cnt.item()) == -5 + B     # inf * |0| is NaN: never close
    assert bool((close == 0).all()) and bool((delta == 0.0).all())


# ---- the models, the handles and the host loop ----

KEYS = ("z", "kkt", "iters", "status", "x0", "u_prev", "nbr", "traj")


def di_model(sc):
    lin = S.lin_of_di(sc)
    return dict(shared=sc.shared, prm=lin["prm"], own=lin["own"], A=sc.A, B=sc.B, x0=sc.x0, u_prev=sc.u_prev, nbr=sc.nbr,
                traj=sc.traj)


@pytest.fixture(scope="module")
def di16():
    return di_model(S.make_di(16, 10, 2, 2))


@pytest.fixture(scope="module")
def ltv7():
    return dict(make_ltv_table(7), mode=PERIODIC)


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


def assert_bytes(got, want, what, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def next_time(m, t):
    return (t + 1) % m["T"] if "table" in m else 0


def host_step(m, ctx, co, t, x0, u_prev, traj, nbr=None):
    """One consensus step on the host's side of the ABI: per inner round lin_window (table only) -> lin_rows ->
    cmpc.solve_mpc -> lin_publish -> consensus_stop, then lin_advance.  Returns the handle's arrays after the step
    and the step's trace."""
    import cmpc

    sh = m["shared"]
    nx, nu, ns, N = sh["nx"], sh["nu"], sh["ns"], sh["N"]
    nbr = m["nbr"] if nbr is None else nbr
    trace = []
    while True:
        A, B, own = S.lin_window(m["table"], t, N, m["mode"]) if "table" in m else (m["A"], m["B"], m["own"])
        qlin, C, h = S.lin_rows(m["prm"], own, nbr, traj)
        z, kkt, iters, status = cmpc.solve_mpc(dict(sh, A=A, B=B, x0=x0, u_prev=u_prev, qlin=qlin, C=C, h=h), ctx)
        traj, close, delta, count = S.lin_publish(m["prm"], z, nx, nu, ns, N, traj, atol=co["atol"], rtol=co["rtol"])
        trace.append(count)
        stop, agreed = S.consensus_stop(trace, co["min_rounds"], co["need"], co["max_rounds"])
        if stop:
            break
    x1, u1, t1 = S.lin_advance(m["prm"], z, nx, nu, ns, N, x0, u_prev, traj)
    assert t1.tobytes() == traj.tobytes()                      # the advance rewrites what was already exchanged
    return dict(z=z, kkt=kkt, iters=iters, status=status, x0=x1, u_prev=u1, traj=t1, nbr=np.asarray(nbr, np.int32),
                inner_rounds=len(trace), agreed=agreed, not_close=np.asarray(trace, np.int32), close=close, delta=delta)


def assert_consensus(H, want, what):
    c = H.consensus()
    assert c["inner_rounds"] == want["inner_rounds"] and c["agreed"] is want["agreed"], (what, c, want["not_close"])
    assert c["not_close"].dtype == np.int32 and np.array_equal(c["not_close"], want["not_close"]), what
    assert c["close"].dtype == np.int32 and np.array_equal(c["close"], want["close"]), what
    assert same(c["delta"], want["delta"]), what


# ---- 2. max_rounds = 1 is a plain round ----

@pytest.mark.parametrize("model", ["di16", "ltv7"])
def test_one_inner_round_equals_a_plain_step(gpu_ctx, request, model):
    m = request.getfixturevalue(model)
    C, P = make_handle(m, gpu_ctx, history=3), make_handle(m, gpu_ctx, history=3)
    for step in range(3):
        assert C.step_consensus(1, min_rounds=1, need=1, max_rounds=1) == (1, 1) and P.step() == 1
        want = handle_state(P)
        assert_bytes(handle_state(C), want, step)
        assert np.isfinite(want["z"]).all()
        if "table" in m:
            assert C.time == P.time == (step + 1) % 7
        c = C.consensus()
        assert c["inner_rounds"] == 1 and not c["agreed"] and len(c["not_close"]) == 1
    hc, hp = C.history(0, 3), P.history(0, 3)
    for k in ("kkt", "iters", "status"):
        assert hc[k].tobytes() == hp[k].tobytes(), k
    C.close()
    P.close()


# ---- 3. consensus steps against the host loop ----

@pytest.mark.parametrize("model,setting", [("di16", "defaults"), ("di16", "capped"), ("ltv7", "defaults")])
def test_consensus_steps_equal_the_host_loop(gpu_ctx, request, model, setting):
    m = request.getfixturevalue(model)
    co = DEFAULTS if setting == "defaults" else CAPPED
    H = make_handle(m, gpu_ctx)
    x0, up, traj, t, steps = m["x0"], m["u_prev"], m["traj"], 0, []
    for step in range(3):
        want = host_step(m, gpu_ctx, co, t, x0, up, traj)
        print(model, setting, "step", step, "not_close", want["not_close"].tolist(), "agreed", want["agreed"],
              "delta max", np.nanmax(want["delta"]))
        assert H.step_consensus(1, **co) == (1, want["inner_rounds"])
        assert_bytes(handle_state(H), want, step)
        assert_consensus(H, want, step)
        t = next_time(m, t)
        if "table" in m:
            assert H.time == t                                   # one stage per consensus step, whatever it ran inside
        steps.append(want)
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    H.close()
    # the host loop's own trace: the comparison above is not vacuous
    assert all((s["status"] == L.CMPC_SOLVED).all() for s in steps)
    if "table" in m:
        return                                                   # (the trace below was worked out for the double integrator)
    if setting == "defaults":
        assert all(s["agreed"] and 3 <= s["inner_rounds"] < 12 for s in steps), [s["not_close"] for s in steps]
        assert any(s["not_close"][1] > 0 for s in steps), [s["not_close"] for s in steps]
    else:
        assert all(s["inner_rounds"] == 3 and not s["agreed"] for s in steps), [s["not_close"] for s in steps]


# ---- 4. behaviour around a step ----

def test_history_log_mixing_and_set_state(gpu_ctx, di16):
    m, sh = di16, di16["shared"]
    H = make_handle(m, gpu_ctx, history=8, log=8)
    a = host_step(m, gpu_ctx, DEFAULTS, 0, m["x0"], m["u_prev"], m["traj"])
    assert H.step_consensus() == (1, a["inner_rounds"])
    assert_bytes(handle_state(H), a, "consensus")
    # a plain round in between: one inner round of the same pieces
    one = dict(DEFAULTS, min_rounds=1, max_rounds=1)
    b = host_step(m, gpu_ctx, one, 0, a["x0"], a["u_prev"], a["traj"])
    assert H.step() == 1
    assert_bytes(handle_state(H), b, "plain")
    assert H.consensus()["inner_rounds"] == a["inner_rounds"]      # still the latest CONSENSUS step
    # the measured state replaces the predicted one
    x0 = b["x0"].copy()
    x0[:, 2] += 0.05
    up = b["u_prev"] + 0.01
    H.set_state(x0, up)
    c = host_step(m, gpu_ctx, DEFAULTS, 0, x0, up, b["traj"])
    d = host_step(m, gpu_ctx, DEFAULTS, 0, c["x0"], c["u_prev"], c["traj"])
    assert H.step_consensus(2) == (2, c["inner_rounds"] + d["inner_rounds"])
    assert_bytes(handle_state(H), d, "two steps in one call")
    assert_consensus(H, d, "two steps in one call")
    # one row per step, with the last inner round's outputs
    assert H.log_range() == (0, 4)
    lg, hist = H.log(), H.history(0, 4)
    for i, r in enumerate((a, b, c, d)):
        state, u, look = S.log_row(r["z"], sh["nx"], sh["nu"], sh["ns"], sh["N"], m["prm"]["ix"])
        assert lg["state"][i].tobytes() == state.tobytes() and lg["u"][i].tobytes() == u.tobytes(), i
        assert lg["look_ahead"][i].tobytes() == look.tobytes(), i
        for k in ("kkt", "iters", "status"):
            assert lg[k][i].tobytes() == r[k].tobytes() and hist[k][i].tobytes() == r[k].tobytes(), (i, k)
    assert (lg["solve_ms"] > 0).all()
    H.close()


def test_reselect_selects_once_per_step(gpu_ctx, di16):
    m = dict(di16)
    p = m["traj"][:, 0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    m["nbr"] = np.argsort(-d2, axis=1, kind="stable")[:, :2].astype(np.int32)    # the farthest: a valid table
    H = make_handle(m, gpu_ctx, reselect=True)
    x0, up, traj = m["x0"], m["u_prev"], m["traj"]
    for step in range(2):
        sel = S.select_neighbours(traj, 2)                   # on the buffer as it stood before the step
        assert (sel != m["nbr"]).any()
        want = host_step(m, gpu_ctx, DEFAULTS, 0, x0, up, traj, nbr=sel)
        assert want["inner_rounds"] >= 3
        assert H.step_consensus() == (1, want["inner_rounds"])
        got = handle_state(H)
        assert np.array_equal(got["nbr"], sel)
        assert_bytes(got, want, step)
        x0, up, traj = want["x0"], want["u_prev"], want["traj"]
    H.close()


def test_step_argument_errors(gpu_ctx, di16):
    from cmpc import CmpcError

    m, lib = di16, gpu_ctx.lib
    H, P = make_handle(m, gpu_ctx), make_handle(m, gpu_ctx)
    nan = float("nan")

    def refused(h, steps, co):
        done, inner = ct.c_int(-7), ct.c_int(-7)
        rc = lib.cmpc_lin_rounds_step_consensus(h, steps, None if co is None else ct.byref(L.cmpc_consensus_opts(*co)),
                                                ct.byref(done), ct.byref(inner))
        return rc == L.CMPC_ERR_ARG and (done.value, inner.value) == (-7, -7)

    assert refused(None, 1, None)
    for steps, co in ((-1, None), (1, (0, 2, 12, 0.01, 1e-5)), (1, (3, 0, 12, 0.01, 1e-5)), (1, (3, 2, 2, 0.01, 1e-5)),
                      (1, (1, 1, 0, 0.01, 1e-5)), (1, (3, 2, 12, -0.01, 1e-5)), (1, (3, 2, 12, nan, 1e-5)),
                      (1, (3, 2, 12, 0.01, -1e-5)), (1, (3, 2, 12, 0.01, nan)), (0, (0, 2, 12, 0.01, 1e-5))):
        assert refused(H.h, steps, co), (steps, co)
        assert lib.cmpc_last_error(gpu_ctx.h)
    with pytest.raises(CmpcError) as e:
        H.step_consensus(1, need=0)
    assert e.value.code == L.CMPC_ERR_ARG
    # the exchange lies inside the step: not on a sharded handle that leaves it to the host
    X = make_handle(m, gpu_ctx, rank=1, world=2, host_exchange=True)
    assert refused(X.h, 1, None) and refused(X.h, 0, None)
    assert X.step() == 1                                         # ... which still runs plain rounds
    X.close()
    # _consensus_read
    o = L.cmpc_consensus_out(None, None, None, -1, None, None)
    assert lib.cmpc_lin_rounds_consensus_read(H.h, ct.byref(o)) == L.CMPC_ERR_ARG
    assert lib.cmpc_lin_rounds_consensus_read(H.h, None) == L.CMPC_ERR_ARG
    assert lib.cmpc_lin_rounds_consensus_read(None, ct.byref(o)) == L.CMPC_ERR_ARG
    c = H.consensus()                                            # before the first consensus step
    assert c["inner_rounds"] == 0 and not c["agreed"] and not c["close"].any() and not c["delta"].any()
    # no steps, NULL options and NULL counters are taken; the handle's next plain step is what it would have been
    assert lib.cmpc_lin_rounds_step_consensus(H.h, 0, None, None, None) == L.CMPC_OK
    assert H.step() == 1 and P.step() == 1
    assert_bytes(handle_state(H), handle_state(P), "after the refused calls")
    assert lib.cmpc_lin_rounds_step_consensus(H.h, 1, None, None, None) == L.CMPC_OK
    c = H.consensus()
    trace = np.full(2, -7, np.int32)                             # cap < inner_rounds: the first cap entries
    o = L.cmpc_consensus_out(None, None, L.iptr(trace), 2, None, None)
    assert lib.cmpc_lin_rounds_consensus_read(H.h, ct.byref(o)) == L.CMPC_OK
    assert c["inner_rounds"] >= 3 and np.array_equal(trace, c["not_close"][:2])
    H.close()
    P.close()


def test_a_solver_error_leaves_the_step_uncounted(gpu_ctx, ltv7):
    """CMPC_FLAG_LPV_AUTO passes create and fails the solver call of a device entry: the error comes back unchanged,
    no step is counted and the time stays."""
    m = ltv7
    H = make_handle(m, gpu_ctx, opts=L.opts(flags=L.CMPC_FLAG_LPV_AUTO), log=2)
    before = handle_state(H)
    done, inner = ct.c_int(-7), ct.c_int(-7)
    rc = gpu_ctx.lib.cmpc_lin_rounds_step_consensus(H.h, 2, None, ct.byref(done), ct.byref(inner))
    assert rc == L.CMPC_ERR_ARG and (done.value, inner.value) == (0, 0)
    assert H.time == 0 and H.log_range() == (0, 0) and H.consensus()["inner_rounds"] == 0
    assert_bytes(handle_state(H), before, "after the error", ("x0", "u_prev", "traj"))
    H.close()


# ---- 5. an agent without a finite solution ----

def test_a_non_finite_agent_publishes_its_previous_row(gpu_ctx):
    m = di_model(S.make_di(6, 10, 2, 2))
    H = make_handle(m, gpu_ctx)
    assert H.step() == 1
    a = handle_state(H)
    bad = a["x0"].copy()
    bad[2, 0] = np.nan
    H.set_state(bad)
    assert H.step_consensus(1, min_rounds=1, need=1, max_rounds=3) == (1, 3)
    e, c = handle_state(H), H.consensus()
    assert not np.isfinite(e["z"][2]).all()
    assert e["traj"][2].tobytes() == a["traj"][2].tobytes() and np.isfinite(e["traj"]).all()
    assert same(e["x0"][2], bad[2]) and e["u_prev"][2].tobytes() == a["u_prev"][2].tobytes()
    assert c["close"][2] == 0 and np.isnan(c["delta"][2])
    assert c["inner_rounds"] == 3 and not c["agreed"] and (c["not_close"] >= 1).all()
    others = [i for i in range(6) if i != 2]
    assert np.isfinite(e["z"][others]).all() and np.isfinite(c["delta"][others]).all()
    assert not np.array_equal(e["traj"][others], a["traj"][others])
    H.close()
