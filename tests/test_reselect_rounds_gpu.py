"""Consensus rounds that re-select their neighbour table on the device (`DIRounds` / `LPVRounds`
`reselect=r`, the round handle's CMPC_ROUNDS_RESELECT) against the same rounds driven from the host:
download the exchange buffer, `scenarios.select_neighbours`, upload the table, `step()`.  Bit-equal."""
import numpy as np
import pytest

from cmpc import scenarios as S

pytestmark = pytest.mark.gpu

DI_FIELDS = ("z", "kkt", "iters", "status", "x0", "u_prev", "traj_all", "nbr")


def wrong_table(n, nb, shift=0):
    """nbr[i, j] = (i + 31 + j + shift) % n: valid indices, never the agent itself, never its nearest."""
    return ((np.arange(n)[:, None] + 31 + np.arange(nb)[None, :] + shift) % n).astype(np.int32)


def di_scenario(wrong=True):
    sc = S.make_di(64, 10, 2)
    # on the CPU the (0, 0) selection of this scenario is its own table, order included
    assert np.array_equal(S.select_neighbours(sc.traj, 2), sc.nbr)
    if wrong:
        sc.nbr = wrong_table(64, 2)
        assert (sc.nbr != S.select_neighbours(sc.traj, 2)).all()
    return sc


def host(t):
    return t.detach().cpu().numpy().copy()


def assert_same(a, b, fields, what):
    for f in fields:
        assert np.array_equal(host(getattr(a, f)), host(getattr(b, f)), equal_nan=True), (what, f)


def host_select(R, nb, window=(0, 0)):
    """The host's way: download traj_all, select, upload into R.nbr."""
    import torch

    sel = S.select_neighbours(host(R.traj_all), nb, window, rows=slice(R.off, R.off + R.B))
    R.nbr.copy_(torch.as_tensor(sel, device=R.nbr.device))
    return sel


@pytest.mark.parametrize("fused,window", [(True, (0, 0)), (False, (0, 0)), (True, (0, 10)), (False, (0, 10))])
def test_di_rounds_reselect_equals_host_driven_loop(gpu_ctx, fused, window):
    import torch

    from cmpc.rounds import DIRounds

    sc = di_scenario()
    dev = DIRounds(sc, ctx=gpu_ctx, fused=fused, reselect=1, reselect_window=window)
    ref = DIRounds(sc, ctx=gpu_ctx, fused=fused)
    first = S.select_neighbours(sc.traj, 2, window)
    assert (host(dev.nbr) != first).any()           # the deliberately wrong table, before the first round
    for rnd in range(4):
        sel = host_select(ref, 2, window)
        dev.step()
        ref.step()
        torch.cuda.synchronize()
        if rnd == 0:
            assert np.array_equal(host(dev.nbr), first)
        assert np.array_equal(host(dev.nbr), sel)
        assert_same(dev, ref, DI_FIELDS, rnd)
    assert np.isfinite(host(dev.z)).all()


def test_di_rounds_reselect_every_third_round(gpu_ctx):
    """reselect = 3 over 7 rounds: the table is replaced at rounds 0, 3 and 6 only — a table spoilt before
    every round stays spoilt on the others."""
    import torch

    from cmpc.rounds import DIRounds

    R = DIRounds(di_scenario(), ctx=gpu_ctx, reselect=3)
    for rnd in range(7):
        spoilt = wrong_table(64, 2, rnd)
        R.nbr.copy_(torch.as_tensor(spoilt, device=R.nbr.device))
        want = S.select_neighbours(host(R.traj_all), 2) if rnd % 3 == 0 else spoilt
        R.step()
        torch.cuda.synchronize()
        assert np.array_equal(host(R.nbr), want), rnd
    R.select_neighbours()                           # the public method: one selection, now
    assert np.array_equal(host(R.nbr), S.select_neighbours(host(R.traj_all), 2))
    R.select_neighbours(window=(0, 10))
    assert np.array_equal(host(R.nbr), S.select_neighbours(host(R.traj_all), 2, (0, 10)))


@pytest.mark.parametrize("wrong", [False, True])
def test_di_rounds_reselect_off_changes_nothing(gpu_ctx, wrong):
    """reselect = 0 is a DIRounds built without the argument: nothing silently repairs a wrong table."""
    import torch

    from cmpc.rounds import DIRounds

    sc = di_scenario(wrong)
    a, b = DIRounds(sc, ctx=gpu_ctx, reselect=0), DIRounds(sc, ctx=gpu_ctx)
    for rnd in range(3):
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert_same(a, b, DI_FIELDS, rnd)
        assert np.array_equal(host(a.nbr), sc.nbr)


def lpv_case(ctx, name, nb):
    """A captured reference run of the existing rounds tests (tests/test_rounds_gpu.py), its table cut to
    `nb` neighbours per agent: lpv_n10_a2 is the smallest population with a neighbour at all (two agents,
    so the selection can only return the other one); lpv_n20_a4 with two of three is a real choice."""
    from test_rounds_gpu import _case

    bp, args, kw, _ = _case(name, ctx)
    n = args[0].shape[0]
    nbr = ((np.arange(n)[:, None] + 1 + np.arange(nb)[None, :]) % n).astype(np.int32)
    return bp, (args[0], args[1], args[2], nbr), kw


LPV_CASES = [("lpv_n10_a2", 1), ("lpv_n20_a4", 2)]


@pytest.mark.parametrize("name,nb", LPV_CASES)
def test_lpv_rounds_reselect_equals_host_driven_loop(gpu_ctx, name, nb):
    import torch

    from cmpc.rounds import LPVRounds

    bp, args, kw = lpv_case(gpu_ctx, name, nb)
    dev = LPVRounds(bp, *args, **kw, reselect=1)
    ref = LPVRounds(bp, *args, **kw)
    for rnd in range(3):
        sel = host_select(ref, nb)
        dev.step(halt=False)
        ref.step(halt=False)
        torch.cuda.synchronize()
        assert np.array_equal(host(dev.nbr), sel)
        assert_same(dev, ref, ("z", "planes", "traj_all", "nbr", "status"), rnd)
    assert np.isfinite(host(dev.z)).all() and np.isfinite(host(dev.planes)).all()


@pytest.mark.parametrize("name,nb", LPV_CASES)
def test_round_handle_reselect_equals_lpvrounds(gpu_ctx, name, nb):
    """Three rounds in one cmpc_lpv_rounds_step call, the selection inside the library's loop."""
    import torch

    from cmpc.rounds import LPVRounds, LPVRoundsHandle

    bp, args, kw = lpv_case(gpu_ctx, name, nb)
    R = LPVRounds(bp, *args, **kw, reselect=1)
    for _ in range(3):
        R.step(halt=False)
    torch.cuda.synchronize()
    H = LPVRoundsHandle(bp, *args, **kw, halt=False, reselect=True)
    assert H.step(3)[0] == 3
    r = H.read()
    assert np.array_equal(r["z"], host(R.z)) and np.array_equal(r["x0"], host(R.x0))
    assert np.array_equal(r["planes"], host(R.planes))
    assert np.array_equal(H.get_traj(), host(R.traj_local))
    H.close()


def test_round_handle_reselect_needs_fewer_neighbours_than_agents(gpu_ctx):
    from test_rounds_gpu import _case

    from cmpc import CmpcError
    from cmpc.rounds import LPVRoundsHandle

    bp, args, kw, _ = _case("lpv_n10_a1", gpu_ctx)    # one agent, no neighbour: nothing to select, still valid
    H = LPVRoundsHandle(bp, *args, **kw, reselect=True)
    assert H.step(1) == (1, 0)
    H.close()
    bp, args, kw, _ = _case("lpv_n10_a2", gpu_ctx)
    two = np.array([[1, 1], [0, 0]], np.int32)        # nb = 2 = n_total
    with pytest.raises(CmpcError):
        LPVRoundsHandle(bp, args[0], args[1], args[2], two, **kw, reselect=True)
