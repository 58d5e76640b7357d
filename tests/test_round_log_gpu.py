"""The rounds' device log (cmpc_round_log_dev, cmpc_lpv_rounds_log_* / cmpc_di_rounds_log_*) on the GPU: a handle
that logs while it runs several rounds in one step call against a second handle stepped one round at a time and
read back after each — every logged value is a copy, so everything is compared bit for bit."""
import ctypes as ct
import os
import time

import numpy as np
import pytest

from conftest import golden

from cmpc import _lib as L
from cmpc import scenarios as S

pytestmark = pytest.mark.gpu

LOG_KEYS = ("state", "u", "look_ahead", "kkt", "iters", "status")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def err_arg(fn, *args, **kw):
    with pytest.raises(L.CmpcError) as e:
        fn(*args, **kw)
    assert e.value.code == L.CMPC_ERR_ARG
    return True


# ---- the two families' cases (as tests/test_rounds_gpu.py and tests/test_di_rounds_handle_gpu.py build them) ----

def lpv_case(name, ctx):
    import cmpc
    from oracle import lpv_ref as R

    d = golden(name)
    N, n, dt = int(d["N"]), int(d["n_agents"]), float(d["dt"])
    g = R.paper_gains()
    bp = cmpc.PlannerLPVBatch(g["Q"], g["Qs"], g["R"], g["dR"], N, dt, R.Track.build("Highway"), g["wq"],
                              R.SCALED_CAR_MODEL, R.scaled_car_limits(float(d["vx_ref"])), ctx=ctx)
    sel = sorted([j for j in range(len(d["step"])) if d["step"][j] == 0], key=lambda j: d["agent"][j])
    args = (d["x0"][sel].copy(), np.stack([d[f"x_last_{j}"] for j in sel]), np.stack([d[f"u_last_{j}"] for j in sel]),
            np.array(R.neighbour_lists(n), np.int32).reshape(n, n - 1))
    kw = dict(u_old=d["u_old"][sel].copy(), traj=d["pose"][sel].copy())
    return bp, args, kw, int(d["steps"])


def lpv_offtrack(ctx):
    """lpv_n10_a2 at step 0 with agent 0's previous prediction off the track (s = NaN in one row)."""
    bp, args, kw, _ = lpv_case("lpv_n10_a2", ctx)
    x_last = args[1].copy()
    x_last[0, 3, 6] = np.nan
    return bp, (args[0], x_last, args[2], args[3]), kw


def lpv_rows(z, N):
    """What the LPV handle logs of a round's z: nx, nu, ns = 9, 2, 3, look_col = 6."""
    return dict(state=z[:, 0:9], u=z[:, 12 * (N + 1):12 * (N + 1) + 2], look_ahead=z[:, 12 * N + 6] - z[:, 6])


def di_rows(z, N, dim):
    """What the DI handle logs: nx = 2 dim, nu = dim, ns = 3, look_col = 0."""
    nxe = 2 * dim + 3
    return dict(state=z[:, 0:2 * dim], u=z[:, nxe * (N + 1):nxe * (N + 1) + dim], look_ahead=z[:, nxe * N] - z[:, 0])


def one_at_a_time(H, rounds, rows):
    """`rounds` single-round steps of handle H; per round the expected log row, read() and get_traj()."""
    per = []
    for _ in range(rounds):
        done = H.step(1)
        assert done in (1, (1, 0)), done
        r = H.read()
        want = dict(rows(r["z"]), kkt=r["kkt"], iters=r["iters"], status=r["status"])
        per.append(dict(want=want, read=r, traj=H.get_traj()))
    return per


def assert_log_rows(lg, first, per):
    """Rows of log dict `lg` (round `first` in row 0) against the per-round expectations."""
    for i in range(len(lg["kkt"])):
        for k in LOG_KEYS:
            assert same(lg[k][i], per[first + i]["want"][k]), (first + i, k)


def assert_same_final_state(a, b):
    ra, rb = a.read(), b.read()
    assert set(ra) == set(rb)
    for k in ra:
        assert same(ra[k], rb[k]), k
    assert same(a.get_traj(), b.get_traj())


# ---- 1, 2: the log of one multi-round step equals stepping one round at a time ----

@pytest.mark.parametrize("name", ["lpv_n10_a2", "lpv_n20_a4"])
def test_lpv_log_equals_one_round_at_a_time(gpu_ctx, name):
    from cmpc.rounds import LPVRoundsHandle

    bp, args, kw, steps = lpv_case(name, gpu_ctx)
    N = bp.N
    A = LPVRoundsHandle(bp, *args, **kw)
    B = LPVRoundsHandle(bp, *args, **kw, log=steps)
    per = one_at_a_time(A, steps, lambda z: lpv_rows(z, N))
    assert B.log_range() == (0, 0)
    assert B.step(steps) == (steps, 0)
    assert B.log_range() == (0, steps)
    lg = B.log()
    assert lg["state"].shape == (steps, A.B, 9) and lg["u"].shape == (steps, A.B, 2)
    assert lg["look_ahead"].shape == lg["kkt"].shape == lg["iters"].shape == lg["status"].shape == (steps, A.B)
    assert lg["solve_ms"].shape == (steps,) and "sep2" not in lg
    assert_log_rows(lg, 0, per)
    assert np.isfinite(lg["state"]).all() and (lg["iters"] > 0).all()
    assert_same_final_state(A, B)               # the log changes no result
    A.close()
    B.close()


DI_SHAPES = [(6, 9, 2, 2), (6, 9, 3, 2), (12, 25, 2, 3)]   # the fused v3 round, the generic kernel, Riccati + LPT


@pytest.mark.parametrize("shape", DI_SHAPES)
def test_di_log_equals_one_round_at_a_time(gpu_ctx, shape):
    from cmpc.rounds import DIRoundsHandle

    sc = S.make_di(*shape)
    n, N, _, dim = shape
    A = DIRoundsHandle(sc, ctx=gpu_ctx)
    B = DIRoundsHandle(sc, ctx=gpu_ctx, history=1, log=3)      # history = 1: the log keeps its own copies
    assert B.lpt == A.lpt == (shape == (12, 25, 2, 3))
    per = one_at_a_time(A, 3, lambda z: di_rows(z, N, dim))
    assert B.step(3) == 3
    assert B.log_range() == (0, 3)
    lg = B.log()
    assert lg["state"].shape == (3, n, 2 * dim) and lg["u"].shape == (3, n, dim)
    assert_log_rows(lg, 0, per)
    assert np.isfinite(lg["state"]).all() and (lg["iters"] > 0).all()
    assert_same_final_state(A, B)
    A.close()
    B.close()


# ---- 3: the ring ----

def test_ring_range_and_argument_errors(gpu_ctx):
    from cmpc.rounds import DIRoundsHandle, LPVRoundsHandle

    sc = S.make_di(6, 9, 2, 2)
    lib = gpu_ctx.lib
    A = DIRoundsHandle(sc, ctx=gpu_ctx)
    per = one_at_a_time(A, 3, lambda z: di_rows(z, 9, 2))
    H = DIRoundsHandle(sc, ctx=gpu_ctx, log=2)
    assert H.log_range() == (0, 0)                              # before any round: (k, 0)
    assert H.log(0, 0)["state"].shape == (0, 6, 4)
    err_arg(H.log, 0, 1)                                        # not yet run
    assert H.step(3) == 3
    assert H.log_range() == (1, 2)                              # capacity 2 over 3 rounds
    assert_log_rows(H.log(1, 2), 1, per)
    assert_log_rows(H.log(), 1, per)                            # the default: everything the ring holds
    assert_log_rows(H.log(2, 1), 2, per)                        # the row before the ring's wrap ...
    assert_log_rows(H.log(1, 1), 1, per)                        # ... and after it
    for first, count in ((0, 1), (0, 3), (3, 1), (2, 2), (-1, 1), (1, -1)):
        err_arg(H.log, first, count)
    z = H.log(3, 0)
    assert z["state"].shape == (0, 6, 4) and z["u"].shape == (0, 6, 2) and z["iters"].shape == (0, 6)
    assert z["solve_ms"].shape == (0,)
    assert lib.cmpc_di_rounds_log_enable(H.h, 2, 0) == L.CMPC_ERR_ARG          # a second enable
    assert lib.cmpc_last_error(gpu_ctx.h)
    H.close()

    # enabling after one round logs from round 1
    H = DIRoundsHandle(sc, ctx=gpu_ctx)
    err_arg(H.log_range)                                        # not enabled
    err_arg(H.log, 0, 0)
    assert H.step(1) == 1
    for capacity, flags in ((0, 0), (-1, 0), (4, 2), (4, -1), (4, 3)):
        assert lib.cmpc_di_rounds_log_enable(H.h, capacity, flags) == L.CMPC_ERR_ARG, (capacity, flags)
    assert lib.cmpc_di_rounds_log_enable(H.h, 4, 0) == L.CMPC_OK
    assert H.log_range() == (1, 0)
    assert H.step(2) == 2
    assert H.log_range() == (1, 2)
    assert_log_rows(H.log(), 1, per)
    err_arg(H.log, 0, 1)                                        # ran before the log was enabled
    H.close()

    # the LPV handle counts its rounds from create too
    bp, args, kw, _ = lpv_case("lpv_n10_a2", gpu_ctx)
    A = LPVRoundsHandle(bp, *args, **kw)
    per = one_at_a_time(A, 2, lambda z: lpv_rows(z, bp.N))
    H = LPVRoundsHandle(bp, *args, **kw)
    err_arg(H.log_range)
    assert H.step(1) == (1, 0)
    for capacity, flags in ((0, 0), (4, 2)):
        assert lib.cmpc_lpv_rounds_log_enable(H.h, capacity, flags) == L.CMPC_ERR_ARG
    assert lib.cmpc_lpv_rounds_log_enable(H.h, 1, 0) == L.CMPC_OK
    assert lib.cmpc_lpv_rounds_log_enable(H.h, 1, 0) == L.CMPC_ERR_ARG
    assert H.log_range() == (1, 0)
    assert H.step(1) == (1, 0)
    assert H.log_range() == (1, 1)
    assert_log_rows(H.log(), 1, per)
    err_arg(H.log, 0, 1)
    err_arg(H.log, 2, 1)
    A.close()
    H.close()

    for fam in ("lpv", "di"):                                   # NULL handles
        assert getattr(lib, f"cmpc_{fam}_rounds_log_enable")(None, 2, 0) == L.CMPC_ERR_ARG
        assert getattr(lib, f"cmpc_{fam}_rounds_log_range")(None, None, None) == L.CMPC_ERR_ARG
        assert getattr(lib, f"cmpc_{fam}_rounds_log_read")(None, 0, 0, None) == L.CMPC_ERR_ARG


# ---- 4: CMPC_LOG_SEPARATION ----

def assert_separation(lg, per, local=slice(None)):
    for r in range(len(per)):
        idx, d2 = S.select_neighbours(per[r]["traj"], 1, (0, 0), rows=local, return_dist2=True)
        assert same(lg["nearest"][r], idx[:, 0]), r
        assert same(lg["sep2"][r], d2[:, 0]), r


def test_separation_di(gpu_ctx):
    from cmpc.rounds import DIRoundsHandle

    sc = S.make_di(6, 9, 2, 2)
    A = DIRoundsHandle(sc, ctx=gpu_ctx)
    per = one_at_a_time(A, 3, lambda z: di_rows(z, 9, 2))
    B = DIRoundsHandle(sc, ctx=gpu_ctx, log=3, log_separation=True)
    assert B.step(3) == 3
    lg = B.log()
    assert lg["nearest"].shape == lg["sep2"].shape == (3, 6) and lg["nearest"].dtype == np.int32
    assert_separation(lg, per)
    assert_log_rows(lg, 0, per)
    for r in range(3):                                          # stage 0 of the buffer is the logged position
        assert same(lg["state"][r][:, :2], per[r]["traj"][:, 0])
    assert_same_final_state(A, B)
    # sep2 / nearest without the flag
    C = DIRoundsHandle(sc, ctx=gpu_ctx, log=1)
    assert C.step(1) == 1
    buf, ibuf = np.zeros(6), np.zeros(6, np.int32)
    for o in (L.cmpc_rounds_log(sep2=L.dptr(buf)), L.cmpc_rounds_log(nearest=L.iptr(ibuf))):
        assert gpu_ctx.lib.cmpc_di_rounds_log_read(C.h, 0, 1, ct.byref(o)) == L.CMPC_ERR_ARG
    assert gpu_ctx.lib.cmpc_di_rounds_log_read(C.h, 0, 1, ct.byref(L.cmpc_rounds_log(kkt=L.dptr(buf)))) == L.CMPC_OK
    assert same(buf, per[0]["want"]["kkt"])
    assert gpu_ctx.lib.cmpc_di_rounds_log_read(C.h, 0, 1, None) == L.CMPC_ERR_ARG
    # a host-exchange shard's buffer is stale when its round ends
    err_arg(DIRoundsHandle, sc, rank=0, world=2, ctx=gpu_ctx, host_exchange=True, log=2, log_separation=True)
    D = DIRoundsHandle(sc, ctx=gpu_ctx, host_exchange=True, log=2, log_separation=True)   # one rank: its own buffer
    assert D.step(2) == 2
    assert_separation(D.log(), per[:2])
    for h in (A, B, C, D):
        h.close()


def test_separation_lpv(gpu_ctx):
    from cmpc.rounds import LPVRoundsHandle

    bp, args, kw, steps = lpv_case("lpv_n20_a4", gpu_ctx)
    A = LPVRoundsHandle(bp, *args, **kw)
    per = one_at_a_time(A, steps, lambda z: lpv_rows(z, bp.N))
    B = LPVRoundsHandle(bp, *args, **kw, log=steps, log_separation=True)
    assert B.step(steps) == (steps, 0)
    lg = B.log()
    assert_separation(lg, per)
    assert_log_rows(lg, 0, per)
    for r in range(steps):
        assert same(lg["state"][r][:, 7:9], per[r]["traj"][:, 0])
    assert_same_final_state(A, B)
    err_arg(LPVRoundsHandle, bp, *args, **kw, rank=0, world=2, host_exchange=True, log=2, log_separation=True)
    A.close()
    B.close()
    bp, args, kw, _ = lpv_case("lpv_n10_a1", gpu_ctx)          # one agent has no other agent
    err_arg(LPVRoundsHandle, bp, *args, **kw, log=2, log_separation=True)


# ---- 5: an agent without a solution ----

def test_agent_without_a_solution_logs_nan_rows(gpu_ctx):
    import cmpc
    from cmpc.rounds import LPVRoundsHandle

    bp, args, kw = lpv_offtrack(gpu_ctx)
    H = LPVRoundsHandle(bp, *args, **kw, halt=False, log=2)
    assert H.step(2) == (2, 1)
    lg = H.log()
    assert H.log_range() == (0, 2)
    for r in range(2):
        assert np.isnan(lg["state"][r, 0]).all() and np.isnan(lg["u"][r, 0]).all() and np.isnan(lg["look_ahead"][r, 0])
        assert lg["status"][r, 0] == cmpc.CMPC_UNSOLVED
        assert np.isfinite(lg["state"][r, 1]).all() and np.isfinite(lg["u"][r, 1]).all()
        assert np.isfinite(lg["look_ahead"][r, 1]) and lg["status"][r, 1] == cmpc.CMPC_SOLVED
    H.close()
    H = LPVRoundsHandle(bp, *args, **kw, log=3)
    assert H.step(3) == (1, 1)                                  # the round that halts the loop ran: it is logged
    assert H.log_range() == (0, 1)
    lg = H.log()
    assert np.isnan(lg["state"][0, 0]).all() and np.isfinite(lg["state"][0, 1]).all()
    H.close()


# ---- 6: host-exchange shards ----

def test_two_host_exchange_shards_log_what_one_handle_logs(gpu_ctx):
    from cmpc.rounds import DIRoundsHandle

    sc = S.make_di(6, 9, 2, 2)
    whole = DIRoundsHandle(sc, ctx=gpu_ctx, log=2)
    parts = [DIRoundsHandle(sc, rank=r, world=2, ctx=gpu_ctx, host_exchange=True, log=2) for r in range(2)]
    for _ in range(2):
        assert whole.step() == 1
        for p in parts:
            assert p.step() == 1
        gathered = np.concatenate([p.get_traj() for p in parts])
        for p in parts:
            p.set_traj(gathered)
    want, got = whole.log(), [p.log() for p in parts]
    assert all(p.log_range() == (0, 2) for p in parts)
    for k in LOG_KEYS:
        both = np.concatenate([g[k] for g in got], axis=1)
        assert same(both, want[k]), k
    assert (want["iters"] > 0).all()
    whole.close()
    for p in parts:
        p.close()


# ---- 7: cmpc_round_log_dev directly ----

DIRECT = dict(nx=5, nu=3, ns=2, N=4, look_col=3)       # no solver has these dimensions: the index arithmetic
BATCH = 7
SENTINEL, ISENTINEL = -7.25, -77


def direct_inputs():
    import torch

    d = DIRECT
    nz = (d["nx"] + d["ns"]) * (d["N"] + 1) + 2 * d["nu"] * d["N"]
    rng = np.random.default_rng(3)
    z = rng.standard_normal((BATCH, nz))
    z[2] = np.nan                                      # an agent the builder flagged
    src = dict(z=z, kkt=rng.uniform(0, 1, BATCH), iters=rng.integers(1, 60, BATCH).astype(np.int32),
               status=rng.choice([1, 2, -2, -10], BATCH).astype(np.int32))
    dev = {k: torch.as_tensor(v, device="cuda") for k, v in src.items()}
    state, u, look = S.log_row(z, **d)
    return src, dev, dict(state=state, u=u, look_ahead=look, kkt=src["kkt"], iters=src["iters"], status=src["status"])


def pools():
    """Destinations carved back to back out of two sentinel-filled pools, so a write past a row shows."""
    import torch

    d = DIRECT
    f = torch.full((BATCH * (d["nx"] + d["nu"] + 2) + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    i = torch.full((2 * BATCH + 16,), ISENTINEL, dtype=torch.int32, device="cuda")
    o, row = 8, {}
    for k, w in (("state", d["nx"]), ("u", d["nu"]), ("look_ahead", 0), ("kkt", 0)):
        row[k] = f[o:o + BATCH * max(w, 1)].view((BATCH, w) if w else (BATCH,))
        o += BATCH * max(w, 1)
    row["iters"], row["status"] = i[8:8 + BATCH], i[8 + BATCH:8 + 2 * BATCH]
    return f, i, row


def assert_direct(row, want, skipped=()):
    for k in LOG_KEYS:
        got = row[k].cpu().numpy()
        if k in skipped:
            assert (got == (ISENTINEL if got.dtype == np.int32 else SENTINEL)).all(), k
        elif k == "look_ahead":                        # NaN - NaN: a NaN, whichever
            assert np.array_equal(got, want[k], equal_nan=True) and same(got[[0, 1, 3, 4, 5, 6]], want[k][[0, 1, 3, 4, 5, 6]])
        else:
            assert same(got, want[k]), k


def test_round_log_dev_against_log_row(gpu_ctx):
    import torch

    from cmpc.rounds import log_round_dev

    src, dev, want = direct_inputs()
    d = DIRECT
    # the wrapper's own allocation: every destination
    row = log_round_dev(dev["z"], **d, kkt=dev["kkt"], iters=dev["iters"], status=dev["status"], ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert set(row) == set(LOG_KEYS)
    assert_direct(row, want)
    assert set(log_round_dev(dev["z"], **d, ctx=gpu_ctx)) == {"state", "u", "look_ahead"}
    # all six into the pools, then each destination NULL in turn
    for skip in (None,) + LOG_KEYS:
        f, i, row = pools()
        given = {k: t for k, t in row.items() if k != skip}
        log_round_dev(dev["z"], **d, row=given, kkt=dev["kkt"], iters=dev["iters"], status=dev["status"], ctx=gpu_ctx)
        torch.cuda.synchronize()
        assert_direct(row, want, skipped=(skip,))
        fh, ih = f.cpu().numpy(), i.cpu().numpy()
        used = BATCH * (d["nx"] + d["nu"] + 2)
        assert (fh[:8] == SENTINEL).all() and (fh[8 + used:] == SENTINEL).all()      # nothing around the rows
        assert (ih[:8] == ISENTINEL).all() and (ih[8 + 2 * BATCH:] == ISENTINEL).all()
    # a skipped destination needs no source
    f, i, row = pools()
    log_round_dev(dev["z"], **d, row={k: row[k] for k in ("state", "u", "look_ahead")}, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert_direct(row, want, skipped=("kkt", "iters", "status"))
    assert log_round_dev(dev["z"][:0], **d, ctx=gpu_ctx)["state"].shape == (0, 5)


def test_round_log_dev_argument_errors_and_empty_batch(gpu_ctx):
    import torch

    from cmpc.solver import _tptr

    src, dev, want = direct_inputs()
    f, i, row = pools()
    lib = gpu_ctx.lib
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = dict(z=_tptr(dev["z"]), kkt=_tptr(dev["kkt"]), iters=_tptr(dev["iters"]), status=_tptr(dev["status"]))

    def call(dims=None, null=(), dst_null=()):
        dd = dict(batch=BATCH, **DIRECT)
        dd.update(dims or {})
        cd = L.cmpc_log_dims(*[dd[k] for k in ("batch", "nx", "nu", "ns", "N", "look_col")])
        cr = L.cmpc_log_row(*[None if k in dst_null else _tptr(row[k]) for k in LOG_KEYS])
        a = {k: (None if k in null else v) for k, v in ptr.items()}
        return lib.cmpc_round_log_dev(None if "ctx" in null else gpu_ctx.h, None if "dims" in null else ct.byref(cd),
                                      a["z"], a["kkt"], a["iters"], a["status"], None if "row" in null else ct.byref(cr),
                                      stream)

    bad = [dict(null=("ctx",)), dict(null=("dims",)), dict(null=("z",)), dict(null=("row",)),
           dict(null=("kkt",)), dict(null=("iters",)), dict(null=("status",)),        # destination set, no source
           dict(dims=dict(batch=-1)), dict(dims=dict(N=0)), dict(dims=dict(nx=0)), dict(dims=dict(nx=13)),
           dict(dims=dict(nu=0)), dict(dims=dict(nu=5)), dict(dims=dict(ns=-1)), dict(dims=dict(ns=5)),
           dict(dims=dict(look_col=-1)), dict(dims=dict(look_col=5))]
    for kw in bad:
        assert call(**kw) == L.CMPC_ERR_ARG, kw
    assert lib.cmpc_last_error(gpu_ctx.h)
    assert call(dims=dict(batch=0)) == L.CMPC_OK                 # no launch
    assert call(null=("kkt",), dst_null=("kkt",)) == L.CMPC_OK   # neither source nor destination
    torch.cuda.synchronize()
    assert_direct(row, want, skipped=("kkt",))
    assert (f.cpu().numpy()[:8] == SENTINEL).all() and (i.cpu().numpy()[:8] == ISENTINEL).all()
    f2, i2, row = pools()
    assert call(dims=dict(batch=0)) == L.CMPC_OK
    torch.cuda.synchronize()
    assert (f2.cpu().numpy() == SENTINEL).all() and (i2.cpu().numpy() == ISENTINEL).all()


# ---- 8: solve_ms ----

def test_solve_ms_is_positive_and_inside_the_step(gpu_ctx):
    """A sanity condition on where the events sit, not a performance bar: every round's solver launch took some
    time, and all of them together no longer than the step call that queued and awaited them."""
    from cmpc.rounds import DIRoundsHandle, LPVRoundsHandle

    bp, args, kw, _ = lpv_case("lpv_n10_a2", gpu_ctx)
    for H in (DIRoundsHandle(S.make_di(6, 9, 2, 2), ctx=gpu_ctx, log=3), LPVRoundsHandle(bp, *args, **kw, log=3)):
        t0 = time.perf_counter()
        done = H.step(3)
        wall_ms = 1e3 * (time.perf_counter() - t0)
        assert done in (3, (3, 0))
        ms = H.log()["solve_ms"]
        print(type(H).__name__, "solve_ms", ms, "step wall ms", wall_ms)
        assert ms.shape == (3,) and np.isfinite(ms).all() and (ms > 0).all()
        assert ms.sum() <= wall_ms
        assert same(H.log(1, 2)["solve_ms"], ms[1:])            # resolved again from the same events
        H.close()


# ---- 9: the MEX gateways ----

def mex_log(call, hd, *rng):
    import mex_harness as MX

    o, err = call([MX.mx_str("rounds_log"), MX.mx(hd)] + [MX.mx(np.array([float(v)])) for v in rng], 1)
    assert err is None, err
    return lambda name: MX.values(MX.field(o[0], name)) if MX.field(o[0], name) else None


def assert_mex_log(get, want, count, B, nx, nu, separation):
    assert get("first")[0] == 0
    assert same(get("state").reshape(count, B, nx), want["state"])
    assert same(get("u").reshape(count, B, nu), want["u"])
    for k in ("look_ahead", "kkt"):
        assert same(get(k).reshape(count, B), want[k]), k
    for k in ("iters", "status"):
        assert np.array_equal(get(k).reshape(count, B), want[k]), k
    ms = get("solve_ms")
    assert ms.shape == (count,) and np.isfinite(ms).all() and (ms > 0).all()
    if separation:
        assert same(get("sep2").reshape(count, B), want["sep2"])
        assert np.array_equal(get("nearest").reshape(count, B), want["nearest"])
    else:
        assert get("sep2") is None and get("nearest") is None


def test_mex_di_rounds_log(gpu_ctx):
    import mex_harness as MX
    from test_di_mex_gpu import call_di, cmd, matlab_structs

    from cmpc.rounds import DIRoundsHandle

    sc = S.make_di(6, 9, 2, 2)
    H = DIRoundsHandle(sc, ctx=gpu_ctx, log=2, log_separation=True)
    assert H.step(2) == 2
    want = H.log()
    H.close()
    P, D, St = matlab_structs(sc)
    out, err = call_di(cmd("rounds_create", MX.mx_struct(P), MX.mx_struct(D), MX.mx_struct(St)), 1)
    assert err is None, err
    hd = MX.values(out[0])
    _, err = call_di(cmd("rounds_log", hd), 1)
    assert err[0] == "cmpc:solve" and "(-1)" in err[1]          # not enabled
    _, err = call_di(cmd("rounds_log_enable", hd, np.array([2.0]), np.array([float(L.CMPC_LOG_SEPARATION)])), 0)
    assert err is None, err
    _, err = call_di(cmd("rounds_log_enable", hd, np.array([2.0])), 0)
    assert err[0] == "cmpc:solve" and "(-1)" in err[1]          # a second enable
    o, err = call_di(cmd("rounds_step", hd, np.array([2.0])), 1)
    assert err is None and MX.values(o[0])[0] == 2, err
    assert_mex_log(mex_log(call_di, hd, 0, 2), want, 2, 6, 4, 2, True)
    assert_mex_log(mex_log(call_di, hd), want, 2, 6, 4, 2, True)                 # the default range
    _, err = call_di(cmd("rounds_log", hd, np.array([1.0]), np.array([2.0])), 1)
    assert err[0] == "cmpc:solve" and "(-1)" in err[1]          # round 2 has not run
    for ps in (cmd("rounds_log", hd, np.array([0.0])), cmd("rounds_log_enable", hd), cmd("rounds_log", np.array([60.0])),
               cmd("rounds_log", hd, np.array([-1.0]), np.array([1.0]))):
        _, err = call_di(ps, 1)
        assert err is not None and err[0] == "cmpc:di:args", err
    _, err = call_di(cmd("rounds_destroy", hd), 0)
    assert err is None


def test_mex_lpv_rounds_log(gpu_ctx):
    import mex_harness as MX
    from test_mex_gpu import _lpv_matlab

    from cmpc.rounds import LPVRoundsHandle

    bp, args, kw, _ = lpv_case("lpv_n10_a2", gpu_ctx)
    H = LPVRoundsHandle(bp, *args, **kw, log=2)
    assert H.step(2) == (2, 0)
    want = H.log()
    H.close()
    P, D, h = _lpv_matlab("lpv_n10_a2")
    St = dict(nbr=h["nbr"].T.astype(float), traj=h["pose"].transpose(2, 1, 0))
    out, err = MX.call_lpv([MX.mx_str("rounds_create"), MX.mx_struct(P), MX.mx_struct(D), MX.mx_struct(St)], 1)
    assert err is None, err
    hd = MX.values(out[0])
    _, err = MX.call_lpv([MX.mx_str("rounds_log_enable"), MX.mx(hd), MX.mx(np.array([2.0])), MX.mx(np.array([0.0]))], 0)
    assert err is None, err
    o, err = MX.call_lpv([MX.mx_str("rounds_step"), MX.mx(hd), MX.mx(np.array([2.0]))], 2)
    assert err is None and MX.values(o[0])[0] == 2 and MX.values(o[1])[0] == 0, err
    assert_mex_log(mex_log(MX.call_lpv, hd, 0, 2), want, 2, 2, 9, 2, False)
    assert_mex_log(mex_log(MX.call_lpv, hd), want, 2, 2, 9, 2, False)
    _, err = MX.call_lpv([MX.mx_str("rounds_log"), MX.mx(hd), MX.mx(np.array([0.0]))], 1)
    assert err[0] == "cmpc:lpv:args"
    _, err = MX.call_lpv([MX.mx_str("rounds_destroy"), MX.mx(hd)], 0)
    assert err is None
