"""The synthetic family's round handle (cmpc_di_rounds_*, cmpc.rounds.DIRoundsHandle) against `DIRounds` on
the same `make_di` scenario: the handle chains the same launches on the same inputs, so every output of every
round is compared bit for bit."""
import ctypes as ct

import numpy as np
import pytest

from cmpc import scenarios as S

pytestmark = pytest.mark.gpu

# (agents, N, nb, dim): the fused DS kernel twice, v3 <6,3,2> (unfused), the generic kernel, and n = N nu = 75:
# the stage-wise Riccati kernel, where the launch order applies (lpt on both sides by the default rule)
SHAPES = [(6, 9, 2, 2), (6, 30, 2, 2), (6, 9, 2, 3), (6, 9, 3, 2), (12, 25, 2, 3)]
RICCATI = (12, 25, 2, 3)


def host(t):
    return t.detach().cpu().numpy().copy()


def rounds_state(R):
    """DIRounds' state in the layout of DIRoundsHandle.read() + get_traj()."""
    import torch

    torch.cuda.synchronize()
    d = {k: host(getattr(R, k)) for k in ("z", "kkt", "iters", "status", "x0", "u_prev", "nbr")}
    d["traj"] = host(R.traj_local)
    return d


def handle_state(H):
    d = H.read()
    d["traj"] = H.get_traj()
    return d


def assert_equal_state(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("shape", SHAPES)
def test_handle_equals_dirounds_every_round(gpu_ctx, shape):
    from cmpc.rounds import DIRounds, DIRoundsHandle

    sc = S.make_di(*shape)
    R = DIRounds(sc, ctx=gpu_ctx)
    H = DIRoundsHandle(sc, ctx=gpu_ctx)
    assert H.lpt == R.lpt == (shape == RICCATI)
    for rnd in range(3):
        R.step()
        want = rounds_state(R)
        assert H.step() == 1
        assert_equal_state(handle_state(H), want, rnd)
        assert np.isfinite(want["z"]).all() and (want["iters"] > 0).all()
    H.close()


def test_launch_order_changes_no_output(gpu_ctx):
    """CMPC_ROUNDS_LPT only changes when an agent runs: the Riccati shape with it off and on."""
    from cmpc.rounds import DIRoundsHandle

    sc = S.make_di(*RICCATI)
    off, on = DIRoundsHandle(sc, ctx=gpu_ctx, lpt=False), DIRoundsHandle(sc, ctx=gpu_ctx, lpt=True)
    for rnd in range(3):
        assert off.step() == 1 and on.step() == 1
        a = handle_state(on)
        assert_equal_state(handle_state(off), a, rnd)
    assert len(set(a["iters"].tolist())) > 1      # the order of the last launch was not the identity's
    off.close()
    on.close()


@pytest.mark.parametrize("shape", [(6, 9, 2, 2), RICCATI])
def test_three_rounds_in_one_step_and_history_ring(gpu_ctx, shape):
    """step(3) = 3 x step(1); history = 2 keeps rounds 1 and 2 of three, round 0 is overwritten."""
    from cmpc import CmpcError
    from cmpc import _lib as L
    from cmpc.rounds import DIRoundsHandle

    sc = S.make_di(*shape)
    one, three = DIRoundsHandle(sc, ctx=gpu_ctx), DIRoundsHandle(sc, ctx=gpu_ctx, history=2)
    with pytest.raises(CmpcError):
        three.history(0, 1)                        # not yet run
    per_round = []
    for _ in range(3):
        assert one.step(1) == 1
        per_round.append(handle_state(one))
    assert three.step(3) == 3
    assert_equal_state(handle_state(three), per_round[2], "step(3)")
    hist = three.history(1, 2)
    for i, rnd in enumerate((1, 2)):
        for k in ("kkt", "iters", "status"):
            assert hist[k][i].tobytes() == per_round[rnd][k].tobytes(), (rnd, k)
    assert three.history(2, 1)["iters"].tobytes() == per_round[2]["iters"].tobytes()
    assert three.history(3, 0)["iters"].shape == (0, shape[0])
    for first, count in ((0, 1), (0, 3), (2, 2), (3, 1), (-1, 1), (1, -1)):
        with pytest.raises(CmpcError) as e:
            three.history(first, count)
        assert e.value.code == L.CMPC_ERR_ARG
    with pytest.raises(CmpcError):
        one.history(1, 1)                          # history = 1: only round 2 is left
    assert one.history(2, 1)["kkt"].tobytes() == per_round[2]["kkt"].tobytes()
    assert three.step(0) == 0
    one.close()
    three.close()


def farthest_table(traj, nb):
    """Each agent's nb farthest agents now: a valid table that the (0, 0) selection must replace."""
    p = traj[:, 0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return np.argsort(-d2, axis=1, kind="stable")[:, :nb].astype(np.int32)


def test_reselect_equals_dirounds_reselect(gpu_ctx):
    from cmpc.rounds import DIRounds, DIRoundsHandle

    sc = S.make_di(6, 9, 2, 2)
    sc.nbr = farthest_table(sc.traj, 2)
    first = S.select_neighbours(sc.traj, 2)
    assert (sc.nbr != first).any(axis=1).all()     # round 0's selection changes every row of the table
    R = DIRounds(sc, ctx=gpu_ctx, reselect=1)
    H = DIRoundsHandle(sc, ctx=gpu_ctx, reselect=True)
    for rnd in range(3):
        R.step()
        want = rounds_state(R)
        assert H.step() == 1
        got = handle_state(H)
        assert_equal_state(got, want, rnd)
        if rnd == 0:
            assert np.array_equal(got["nbr"], first)
    H.close()


def test_two_host_exchange_shards_equal_one_handle(gpu_ctx):
    """3 + 3 agents behind two handles on one device, the test doing the exchange, against one handle of 6."""
    from cmpc import CmpcError
    from cmpc.rounds import DIRoundsHandle

    sc = S.make_di(6, 9, 2, 2)
    whole = DIRoundsHandle(sc, ctx=gpu_ctx)
    parts = [DIRoundsHandle(sc, rank=r, world=2, ctx=gpu_ctx, host_exchange=True) for r in range(2)]
    with pytest.raises(CmpcError):
        parts[0].step(2)                           # one round per step: the exchange is the host's
    for rnd in range(2):
        assert whole.step() == 1
        want = handle_state(whole)
        got = [p.step() and handle_state(p) for p in parts]
        for k in want:
            both = np.concatenate([g[k] for g in got])
            assert both.tobytes() == want[k].tobytes(), (rnd, k)
        gathered = np.concatenate([g["traj"] for g in got])
        for p in parts:
            p.set_traj(gathered)
    with pytest.raises(ValueError):
        parts[0].set_traj(gathered[:3])
    whole.close()
    for p in parts:
        p.close()


def raw_create(ctx, sc, dims=None, prm=None, init=None, opts=None, null=()):
    """cmpc_di_rounds_create on scenario `sc` with fields replaced; returns (rc, handle)."""
    from cmpc import _lib as L
    from cmpc.solver import _weights

    n = sc.n_agents
    d = dict(n_total=n, batch=n, self_offset=0, N=sc.N, nb=sc.nb, flags=0, history=1)
    d.update(dims or {})
    cd = L.cmpc_di_rounds_dims(*[d[k] for k in ("n_total", "batch", "self_offset", "N", "nb", "flags", "history")])
    p = dict(sc.params)
    p.update(prm or {})
    cp = L.cmpc_di_params(int(p["dim"]), *(float(p[k]) for k in ("v_ref", "q_v", "q_lane", "hw", "min_vel", "max_vel",
                                                                  "min_dist", "wq")))
    w, keep = _weights(sc.shared)
    a = dict(A=L.f64(sc.A), B=L.f64(sc.B), x0=L.f64(sc.x0), u_prev=L.f64(sc.u_prev), lane=L.f64(sc.lane),
             nbr=L.i32(sc.nbr), traj=L.f64(sc.traj))
    a.update(init or {})
    ci = L.cmpc_di_rounds_init(*[None if k in null else (L.iptr(a[k]) if k == "nbr" else L.dptr(a[k]))
                                 for k in ("A", "B", "x0", "u_prev", "lane", "nbr", "traj")])
    co = L.opts(None, None, (opts or {}).get("flags", 0))
    h = ct.c_void_p()
    ref = lambda name, v: None if name in null else ct.byref(v)  # noqa: E731
    rc = ctx.lib.cmpc_di_rounds_create(ctx.h, ref("prm", cp), ref("w", w), ref("dims", cd), ref("init", ci),
                                       ref("opts", co), None if "out" in null else ct.byref(h))
    return rc, h


def test_create_argument_errors(gpu_ctx):
    from cmpc import _lib as L

    sc = S.make_di(6, 9, 2, 2)
    lib = gpu_ctx.lib
    rc, h = raw_create(gpu_ctx, sc, null=("opts",))                 # opts may be NULL
    assert rc == L.CMPC_OK and h.value
    assert lib.cmpc_di_rounds_destroy(h) == L.CMPC_OK
    rc, h = raw_create(gpu_ctx, sc, dims=dict(flags=L.CMPC_ROUNDS_NO_HALT, history=0))   # accepted, no effect; 0 -> 1
    assert rc == L.CMPC_OK
    assert lib.cmpc_di_rounds_destroy(h) == L.CMPC_OK
    far = sc.nbr.copy()
    far[4, 1] = 6
    neg = sc.nbr.copy()
    neg[0, 0] = -1
    bad = [dict(null=("prm",)), dict(null=("w",)), dict(null=("dims",)), dict(null=("init",)), dict(null=("out",)),
           dict(null=("A",)), dict(null=("B",)), dict(null=("x0",)), dict(null=("u_prev",)), dict(null=("lane",)),
           dict(null=("nbr",)), dict(null=("traj",)),
           dict(dims=dict(batch=0)), dict(dims=dict(batch=7)), dict(dims=dict(self_offset=-1)),
           dict(dims=dict(batch=3, self_offset=4, flags=L.CMPC_ROUNDS_HOST_EXCHANGE)),
           dict(dims=dict(N=0)), dict(prm=dict(dim=1)), dict(prm=dict(dim=4)),
           dict(dims=dict(nb=-1)), dict(dims=dict(nb=13)),
           dict(init=dict(nbr=far)), dict(init=dict(nbr=neg)),
           dict(dims=dict(batch=3)),                                  # sharded: no communicator, no host exchange
           dict(dims=dict(history=-1)), dict(dims=dict(flags=16)), dict(dims=dict(flags=-1)),
           dict(dims=dict(nb=6, flags=L.CMPC_ROUNDS_RESELECT)),       # selects nb < n_total
           dict(opts=dict(flags=1 << 20))]
    for kw in bad:
        rc, h = raw_create(gpu_ctx, sc, **kw)
        assert rc == L.CMPC_ERR_ARG and not h.value, kw
        assert lib.cmpc_last_error(gpu_ctx.h)
    rc, h = raw_create(gpu_ctx, sc, dims=dict(batch=3, self_offset=3, flags=L.CMPC_ROUNDS_HOST_EXCHANGE))
    assert rc == L.CMPC_OK                                          # a valid shard
    assert lib.cmpc_di_rounds_destroy(h) == L.CMPC_OK
    for fn, args in ((lib.cmpc_di_rounds_step, (None, 1, None)), (lib.cmpc_di_rounds_read, (None, None)),
                     (lib.cmpc_di_rounds_history, (None, 0, 0, None, None, None)),
                     (lib.cmpc_di_rounds_get_traj, (None, None)), (lib.cmpc_di_rounds_set_traj, (None, None))):
        assert fn(*args) == L.CMPC_ERR_ARG
    assert lib.cmpc_di_rounds_destroy(None) == L.CMPC_OK


def test_solver_refusal_comes_from_the_first_step(gpu_ctx):
    """The handle does not duplicate the solver's rules: both wave flags at once pass create and fail the step
    with the solver's own code."""
    from cmpc import _lib as L

    sc = S.make_di(6, 9, 2, 2)
    rc, h = raw_create(gpu_ctx, sc, opts=dict(flags=L.CMPC_FLAG_ONE_WAVE | L.CMPC_FLAG_TWO_WAVES))
    assert rc == L.CMPC_OK
    done = ct.c_int(-1)
    assert gpu_ctx.lib.cmpc_di_rounds_step(h, 2, ct.byref(done)) == L.CMPC_ERR_ARG and done.value == 0
    assert gpu_ctx.lib.cmpc_last_error(gpu_ctx.h)
    with pytest.raises(L.CmpcError):
        gpu_ctx.check(gpu_ctx.lib.cmpc_di_rounds_history(h, 0, 1, None, None, None))   # no round has run
    assert gpu_ctx.lib.cmpc_di_rounds_destroy(h) == L.CMPC_OK
