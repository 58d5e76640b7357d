"""Consensus steps on the LPV round handles on the device (cmpc_lpv_publish_dev, cmpc_lpv_rounds_step_consensus /
_consensus_read): the publish kernel against its numpy statement and against the linear family's kernel, a one-round
consensus step against a plain round, consensus steps against the torch-driven loop of the same pieces, the handle's
behaviour around a step, the halt rule, the argument errors and a solver error."""
import ctypes as ct

import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S
from lpv_consensus_cases import (ATOL_T, DEFAULTS, PLANTS, PUBLISH_SHAPES, golden_case, handle_args, nz_of,
                                 publish_instance, threshold_instance)

pytestmark = pytest.mark.gpu

CAPPED = dict(min_rounds=1, need=1, max_rounds=3, atol=1e-7, rtol=0.0)
ONE = dict(min_rounds=1, need=1, max_rounds=1)
LPV = dict(ix=7, iy=8, min_dist=0.25, wq=5.0)
SENTINEL = 7.0
KEYS = ("z", "kkt", "iters", "status", "x0", "planes", "traj")


def dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy().copy()


def same(a, b):
    """Finite entries bit for bit, NaNs in the same places (their payloads may differ between host and device)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.where(nan, 0.0, a).tobytes() == np.where(nan, 0.0, b).tobytes()


# ---- 1. the publish kernel ----

def run_publish(ctx, shape, inst, atol, rtol, skip=(), lin=False):
    """cmpc_lpv_publish_dev (``lin``: cmpc_lin_publish_dev with the LPV constants) on sentinel-filled outputs, the
    counts zeroed as the library does; ``skip``: arguments passed as NULL.  Returns dict(traj_local, close, delta,
    counts) of host arrays (None where skipped)."""
    import torch
    from cmpc.rounds import lin_publish_dev, lpv_publish_dev

    N, B, n, off = shape
    z, traj, status, _ = inst
    out = dict(close=torch.full((B,), -5, dtype=torch.int32, device="cuda"),
               delta=torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda"),
               counts=torch.zeros(2, dtype=torch.int32, device="cuda"))
    tl = torch.full((B, N + 1, 2), SENTINEL, dtype=torch.float64, device="cuda")
    arg = {k: None if k in skip else v for k, v in out.items()}
    if lin:
        one = out["counts"][:1]
        lin_publish_dev(LPV, dev(z), 9, 2, 3, N, dev(traj), tl, atol=atol, rtol=rtol, self_offset=off, ctx=ctx,
                        close=arg["close"], delta=arg["delta"], not_close=one)
    else:
        lpv_publish_dev(dev(z), N, dev(traj), tl, status=None if "status" in skip else dev(status, torch.int32),
                        atol=atol, rtol=rtol, self_offset=off, ctx=ctx, **arg)
    torch.cuda.synchronize()
    for k in skip:                                           # a skipped output's buffer was never handed over
        if k != "status":
            assert bool((out[k] == (0 if k == "counts" else -5 if k == "close" else SENTINEL)).all())
    return dict(traj_local=host(tl), **{k: None if k in skip else host(v) for k, v in out.items()})


def check_publish(ctx, shape, inst, atol, rtol, what):
    N, B, n, off = shape
    z, traj, status, _ = inst
    tl, close, delta, not_close, bad = S.lpv_publish(z, N, traj, status, atol=atol, rtol=rtol, self_offset=off)
    got = run_publish(ctx, shape, inst, atol, rtol)
    assert got["traj_local"].tobytes() == tl.tobytes(), what  # copies on both sides: NaN payloads included
    assert got["close"].dtype == np.int32 and np.array_equal(got["close"], close), what
    assert same(got["delta"], delta), what
    assert got["counts"].tolist() == [not_close, bad], what
    if B > 1:
        assert 0 < not_close < B, what                       # both verdicts occur
    # the linear family's kernel with ix = 7, iy = 8, nx = 9, ns = 3, nu = 2: byte for byte
    lin = run_publish(ctx, shape, inst, atol, rtol, lin=True)
    assert lin["traj_local"].tobytes() == got["traj_local"].tobytes(), what
    assert lin["close"].tobytes() == got["close"].tobytes() and lin["delta"].tobytes() == got["delta"].tobytes(), what
    assert lin["counts"].tolist() == [not_close, 0], what
    return got


@pytest.mark.parametrize("shape", PUBLISH_SHAPES)
def test_publish_kernel_equals_lpv_publish_and_the_linear_kernel(gpu_ctx, shape):
    for plant in PLANTS:
        got = check_publish(gpu_ctx, shape, publish_instance(shape, plant), 0.01, 1e-5, plant)
    check_publish(gpu_ctx, shape, threshold_instance(shape), ATOL_T, 0.0, "threshold")
    # each optional output alone as NULL: the others are what they were; status NULL: counts[1] untouched
    inst = publish_instance(shape, PLANTS[-1])
    for skip in ("close", "delta", "counts", "status"):
        part = run_publish(gpu_ctx, shape, inst, 0.01, 1e-5, skip=(skip,))
        for k in ("traj_local", "close", "delta", "counts"):
            if k == skip:
                continue
            want = got[k]
            if skip == "status" and k == "counts":
                want = np.array([got[k][0], 0], np.int32)
            assert same(part[k], want), (skip, k)


def test_publish_argument_errors(gpu_ctx):
    import torch
    from cmpc.solver import _tptr

    N, B, n = 3, 2, 4
    z = torch.zeros((B, nz_of(N)), dtype=torch.float64, device="cuda")
    traj = torch.zeros((n, N + 1, 2), dtype=torch.float64, device="cuda")
    status = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    tl = torch.full((B, N + 1, 2), SENTINEL, dtype=torch.float64, device="cuda")
    close = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    delta = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
    cnt = torch.full((2,), -5, dtype=torch.int32, device="cuda")

    def call(dims=None, atol=0.01, rtol=1e-5, null=()):
        d = dict(batch=B, N=N, nb=0, self_offset=1)
        d.update(dims or {})
        cd = L.cmpc_di_dims(*[d[k] for k in ("batch", "N", "nb", "self_offset")])
        P = lambda k, t: None if k in null else _tptr(t)          # noqa: E731
        return gpu_ctx.lib.cmpc_lpv_publish_dev(gpu_ctx.h, None if "dims" in null else ct.byref(cd), P("z", z),
                                                P("traj_all", traj), _tptr(status), atol, rtol, P("traj_local", tl),
                                                _tptr(close), _tptr(delta), _tptr(cnt), None)

    bad = [dict(dims=dict(N=0)), dict(dims=dict(batch=-1)), dict(dims=dict(self_offset=-1)), dict(atol=-1e-300),
           dict(atol=float("nan")), dict(rtol=-1.0), dict(rtol=float("nan")), dict(atol=float("-inf"))] + \
          [dict(null=(k,)) for k in ("dims", "z", "traj_all", "traj_local")]
    for kw in bad:
        assert call(**kw) == L.CMPC_ERR_ARG, kw
        assert gpu_ctx.lib.cmpc_last_error(gpu_ctx.h)
    assert gpu_ctx.lib.cmpc_lpv_publish_dev(None, None, None, None, None, 0.01, 1e-5, None, None, None, None,
                                            None) == L.CMPC_ERR_ARG
    assert call(dims=dict(batch=0)) == L.CMPC_OK                 # no launch
    torch.cuda.synchronize()
    assert bool((tl == SENTINEL).all()) and bool((close == -5).all()) and bool((delta == SENTINEL).all())
    assert cnt.tolist() == [-5, -5]
    assert call(dims=dict(nb=-3), atol=float("inf"), rtol=float("inf")) == L.CMPC_OK   # nb is not read; +inf is allowed
    torch.cuda.synchronize()
    assert bool((tl == 0.0).all()) and cnt.tolist() == [-5 + B, -5 + B]   # inf * |0| is NaN: never close; status -3
    assert bool((close == 0).all()) and bool((delta == 0.0).all())


# ---- the handles ----

@pytest.fixture(scope="module")
def cases():
    return {name: golden_case(name) for name in ("lpv_n10_a2", "lpv_n10_a1", "lpv_n30_a3", "lpv_n10_lowspeed")}


def handle_state(H):
    d = H.read()
    d["traj"] = H.get_traj()
    return d


def torch_state(R):
    import torch

    torch.cuda.synchronize()
    d = dict(z=host(R.z), kkt=host(R.kkt), iters=host(R.iters), status=host(R.status), x0=host(R.x0),
             traj=host(R.traj_local))
    d["planes"] = host(R.planes)[..., :R.nb]
    return d


def assert_state(got, want, what, keys=KEYS, solved=None):
    """``solved``: the agents whose kkt and iters are compared (default: all; an agent the builder flagged has its
    status and z set by the library, and nothing defines the other two)."""
    for k in keys:
        if solved is not None and k in ("kkt", "iters"):
            assert same(got[k][solved], want[k][solved]), (what, k)
        else:
            assert same(got[k], want[k]), (what, k)


def assert_consensus(H, R, what):
    c = H.consensus()
    assert c["inner_rounds"] == len(R.trace) and c["agreed"] is R.agreed, (what, c, R.trace)
    assert c["not_close"].dtype == np.int32 and c["not_close"].tolist() == list(R.trace), what
    assert c["close"].dtype == np.int32 and np.array_equal(c["close"], host(R.close)), what
    assert same(c["delta"], host(R.delta)), what


# ---- 2. max_rounds = 1 is a plain round ----

@pytest.mark.parametrize("name,steps", [("lpv_n10_a2", None), ("lpv_n10_lowspeed", 3)])
def test_one_inner_round_equals_a_plain_step(gpu_ctx, cases, name, steps):
    from cmpc.rounds import LPVRoundsHandle

    bp, args, kw = handle_args(cases[name], gpu_ctx)
    steps = cases[name]["steps"] if steps is None else steps
    assert steps >= 2 and steps <= 4                             # (the log below holds every step)
    C, P = LPVRoundsHandle(bp, *args, **kw, log=4), LPVRoundsHandle(bp, *args, **kw, log=4)
    for step in range(steps):                                    # the first is the last_rows transition
        assert C.step_consensus(1, **ONE) == (1, 1, 0) and P.step(1) == (1, 0)
        want = handle_state(P)
        assert_state(handle_state(C), want, step)
        assert np.isfinite(want["z"]).all()
        c = C.consensus()
        assert c["inner_rounds"] == 1 and not c["agreed"] and len(c["not_close"]) == 1
    assert C.log_range() == P.log_range() == (0, steps)
    lc, lp = C.log(), P.log()
    for k in lp:
        if k != "solve_ms":
            assert lc[k].tobytes() == lp[k].tobytes(), k
    C.close()
    P.close()


# ---- 3. consensus steps against the torch loop ----

@pytest.mark.parametrize("name,setting", [("lpv_n10_a2", "defaults"), ("lpv_n10_a2", "capped"), ("lpv_n10_a1", "defaults"),
                                          ("lpv_n30_a3", "defaults")])
def test_consensus_steps_equal_the_torch_loop(gpu_ctx, cases, name, setting):
    from cmpc.rounds import LPVRounds, LPVRoundsHandle

    co = DEFAULTS if setting == "defaults" else CAPPED
    bp, args, kw = handle_args(cases[name], gpu_ctx)
    R, H = LPVRounds(bp, *args, **kw), LPVRoundsHandle(bp, *args, **kw)
    runs = []
    for step in range(3):
        inner, agreed = R.step_consensus(**co)
        want = torch_state(R)
        runs.append(dict(trace=list(R.trace), agreed=agreed, inner=inner, status=want["status"], delta=host(R.delta)))
        print(name, setting, "step", step, "not_close", R.trace, "agreed", agreed, "delta", runs[-1]["delta"].tolist())
        assert H.step_consensus(1, **co) == (1, inner, 0)
        assert_state(handle_state(H), want, step)
        assert_consensus(H, R, step)
    H.close()
    # the torch loop's own trace: the comparison above is not vacuous
    assert all((r["status"] == L.CMPC_SOLVED).all() for r in runs), [r["status"] for r in runs]
    assert all(r["trace"][0] > 0 for r in runs)
    if setting == "defaults":
        assert all(r["agreed"] and 3 <= r["inner"] < 12 for r in runs), [r["trace"] for r in runs]
        if name == "lpv_n10_a1":                                 # no neighbour: nothing couples the inner rounds
            assert all(r["inner"] == 3 and r["delta"].tolist() == [0.0] for r in runs), runs
    else:
        assert all(r["inner"] == 3 and not r["agreed"] for r in runs), [r["trace"] for r in runs]


# ---- 4. behaviour around a step ----

def test_mixing_log_and_the_latest_consensus_step(gpu_ctx, cases):
    from cmpc.rounds import LPVRounds, LPVRoundsHandle

    bp, args, kw = handle_args(cases["lpv_n10_a2"], gpu_ctx)
    R, H = LPVRounds(bp, *args, **kw), LPVRoundsHandle(bp, *args, **kw, log=8)
    rows = []
    inner, _ = R.step_consensus()
    assert H.step_consensus() == (1, inner, 0)
    assert_state(handle_state(H), torch_state(R), "consensus")
    rows.append(torch_state(R))
    first = (inner, list(R.trace))
    R.step()                                                     # a plain round in between
    assert H.step(1) == (1, 0)
    assert_state(handle_state(H), torch_state(R), "plain")
    rows.append(torch_state(R))
    c = H.consensus()                                            # still the latest CONSENSUS step
    assert (c["inner_rounds"], c["not_close"].tolist()) == first
    total = 0
    for _ in range(2):
        total += R.step_consensus()[0]
        rows.append(torch_state(R))
    assert H.step_consensus(2) == (2, total, 0)
    assert_state(handle_state(H), torch_state(R), "two steps in one call")
    assert_consensus(H, R, "two steps in one call")
    # one row per step, with the last inner round's outputs
    assert H.log_range() == (0, 4)
    lg = H.log()
    for i, r in enumerate(rows):
        state, u, look = S.log_row(r["z"], 9, 2, 3, bp.N, 6)
        assert lg["state"][i].tobytes() == state.tobytes() and lg["u"][i].tobytes() == u.tobytes(), i
        assert lg["look_ahead"][i].tobytes() == look.tobytes(), i
        for k in ("kkt", "iters", "status"):
            assert lg[k][i].tobytes() == r[k].tobytes(), (i, k)
    assert (lg["solve_ms"] > 0).all()
    H.close()


def test_reselect_selects_once_per_step(gpu_ctx, cases):
    """Three agents, one neighbour each, the table's first content the FARTHEST other agent: every step selects on
    the exchange buffer as it stood before the step, once."""
    from cmpc.rounds import LPVRounds, LPVRoundsHandle

    bp, args, kw = handle_args(cases["lpv_n30_a3"], gpu_ctx)
    p = kw["traj"][:, 0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    far = np.argsort(-d2, axis=1, kind="stable")[:, :1].astype(np.int32)
    args = args[:3] + (far,)
    R = LPVRounds(bp, *args, **kw, reselect=1)
    H = LPVRoundsHandle(bp, *args, **kw, reselect=True)
    for step in range(2):
        before = host(R.traj_all)
        sel = S.select_neighbours(before, 1)
        inner, _ = R.step_consensus()
        assert inner >= 3
        assert np.array_equal(host(R.nbr), sel)                  # one selection, on the buffer before the step
        if step == 0:
            assert (sel != far).any()
        assert H.step_consensus() == (1, inner, 0)
        assert_state(handle_state(H), torch_state(R), step)
        assert_consensus(H, R, step)
    H.close()


# ---- 5. the halt rule ----

def offtrack(case, ctx):
    """lpv_n10_a2 with agent 0's previous prediction off the track (s = NaN in one row): status -10, z not finite."""
    bp, args, kw = handle_args(case, ctx)
    args[1][0, 3, 6] = np.nan
    return bp, args, kw


def test_an_infeasible_agent_halts_the_step_and_the_call(gpu_ctx, cases):
    from cmpc.rounds import InfeasibleRound, LPVRounds, LPVRoundsHandle

    bp, args, kw = offtrack(cases["lpv_n10_a2"], gpu_ctx)
    H, P = LPVRoundsHandle(bp, *args, **kw), LPVRoundsHandle(bp, *args, **kw)
    assert H.step_consensus(3) == (1, 1, 1)                      # one inner round, one step, one infeasible agent
    assert P.step(3) == (1, 1)
    assert_state(handle_state(H), handle_state(P), "halted", solved=[1])
    c = H.consensus()
    assert c["inner_rounds"] == 1 and not c["agreed"] and c["close"][0] == 0 and np.isnan(c["delta"][0])
    H.close()
    P.close()
    R = LPVRounds(bp, *args, **kw)
    with pytest.raises(InfeasibleRound) as ei:
        R.step_consensus()
    assert ei.value.count == 1 and len(R.trace) == 1 and R.last_rows == bp.N   # raised after the step completed


def test_without_the_halt_the_infeasible_agent_stays_put(gpu_ctx, cases):
    from cmpc.rounds import LPVRounds, LPVRoundsHandle

    bp, args, kw = offtrack(cases["lpv_n10_a2"], gpu_ctx)
    H = LPVRoundsHandle(bp, *args, **kw, halt=False)
    assert H.step_consensus(2, min_rounds=1, need=1, max_rounds=3) == (2, 6, 1)
    e, c = handle_state(H), H.consensus()
    assert e["status"].tolist() == [L.CMPC_UNSOLVED, L.CMPC_SOLVED]
    assert e["x0"][0].tobytes() == args[0][0].tobytes() and e["traj"][0].tobytes() == kw["traj"][0].tobytes()
    assert c["close"][0] == 0 and np.isnan(c["delta"][0])
    assert c["inner_rounds"] == 3 and not c["agreed"] and (c["not_close"] >= 1).all()
    assert np.isfinite(e["z"][1]).all() and np.isfinite(c["delta"][1]) and not np.isfinite(e["z"][0]).all()
    assert np.isfinite(e["traj"]).all()
    assert not np.array_equal(e["x0"][1], args[0][1])
    H.close()
    R = LPVRounds(bp, *args, **kw)                               # the torch loop: the same two steps
    for _ in range(2):
        assert R.step_consensus(min_rounds=1, need=1, max_rounds=3, halt=False) == (3, False)
    assert_state(e, torch_state(R), "torch loop", solved=[1])
    assert R.infeasible() == 1


# ---- 6. the step's argument errors ----

def test_step_argument_errors(gpu_ctx, cases):
    from cmpc import CmpcError
    from cmpc.rounds import LPVRoundsHandle

    lib = gpu_ctx.lib
    bp, args, kw = handle_args(cases["lpv_n10_a2"], gpu_ctx)
    H, P = LPVRoundsHandle(bp, *args, **kw), LPVRoundsHandle(bp, *args, **kw)
    nan = float("nan")

    def refused(h, steps, co):
        done, inner, bad = ct.c_int(-7), ct.c_int(-7), ct.c_int(-7)
        rc = lib.cmpc_lpv_rounds_step_consensus(h, steps, None if co is None else ct.byref(L.cmpc_consensus_opts(*co)),
                                                ct.byref(done), ct.byref(inner), ct.byref(bad))
        return rc == L.CMPC_ERR_ARG and (done.value, inner.value, bad.value) == (-7, -7, -7)

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
    X = LPVRoundsHandle(bp, *args, **kw, rank=1, world=2, host_exchange=True)
    assert refused(X.h, 1, None) and refused(X.h, 0, None)
    assert X.step(1) == (1, 0)                                   # ... which still runs plain rounds
    X.close()
    # _consensus_read
    o = L.cmpc_consensus_out(None, None, None, -1, None, None)
    assert lib.cmpc_lpv_rounds_consensus_read(H.h, ct.byref(o)) == L.CMPC_ERR_ARG
    assert lib.cmpc_lpv_rounds_consensus_read(H.h, None) == L.CMPC_ERR_ARG
    assert lib.cmpc_lpv_rounds_consensus_read(None, ct.byref(o)) == L.CMPC_ERR_ARG
    c = H.consensus()                                            # before the first consensus step
    assert c["inner_rounds"] == 0 and not c["agreed"] and not c["close"].any() and not c["delta"].any()
    # no steps, NULL options and NULL counters are taken; the handle's next plain step is what it would have been
    assert lib.cmpc_lpv_rounds_step_consensus(H.h, 0, None, None, None, None) == L.CMPC_OK
    assert H.step(1) == (1, 0) and P.step(1) == (1, 0)
    assert_state(handle_state(H), handle_state(P), "after the refused calls")
    assert lib.cmpc_lpv_rounds_step_consensus(H.h, 1, None, None, None, None) == L.CMPC_OK
    c = H.consensus()
    trace = np.full(3, -7, np.int32)                             # cap < inner_rounds: the first cap entries
    o = L.cmpc_consensus_out(None, None, L.iptr(trace), 2, None, None)
    assert lib.cmpc_lpv_rounds_consensus_read(H.h, ct.byref(o)) == L.CMPC_OK
    assert c["inner_rounds"] >= 3 and np.array_equal(trace[:2], c["not_close"][:2]) and trace[2] == -7
    H.close()
    P.close()


# ---- 7. a solver error ----

def test_a_solver_error_leaves_the_step_uncounted(gpu_ctx, cases):
    """CMPC_FLAG_LANE passes create (a known flag) and fails the solver call (no lane-per-agent kernel for the LPV
    agents' dimensions): the code comes back unchanged, no step is counted, the log stays empty and the state is
    untouched — a plain step after the flag is gone (a twin without it) starts from the same state."""
    from cmpc.rounds import LPVRoundsHandle

    bp, args, kw = handle_args(cases["lpv_n10_a2"], gpu_ctx)
    good = bp.opts.flags
    bp.opts.flags = good | L.CMPC_FLAG_LANE
    H = LPVRoundsHandle(bp, *args, **kw, log=2)                  # (the handle copies the options at create)
    bp.opts.flags = good
    before = handle_state(H)
    plain = ct.c_int(-7)
    rc_plain = gpu_ctx.lib.cmpc_lpv_rounds_step(H.h, 1, ct.byref(plain), None)
    done, inner, bad = ct.c_int(-7), ct.c_int(-7), ct.c_int(-7)
    rc = gpu_ctx.lib.cmpc_lpv_rounds_step_consensus(H.h, 2, None, ct.byref(done), ct.byref(inner), ct.byref(bad))
    assert rc == rc_plain == L.CMPC_ERR_UNSUPPORTED and (done.value, inner.value, bad.value) == (0, 0, 0)
    assert H.log_range() == (0, 0) and H.consensus()["inner_rounds"] == 0
    assert_state(handle_state(H), before, "after the error", ("x0", "traj"))
    H.close()
