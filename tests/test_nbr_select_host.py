"""CPU checks of `scenarios.select_neighbours`, the numpy statement of the device neighbour selection
(cmpc_nbr_select_dev): score = min over the window's stages of dx*dx + dy*dy, a NaN score counts as +inf,
order by (score, index), the agent itself left out by index and never by distance."""
import numpy as np
import pytest

from cmpc import scenarios as S


def lattice(n=65, N=2, seed=3):
    """n agents on the integer lattice {0..3}^2 at every stage: many exact zero and equal scores, and
    agents on the own agent's point."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, size=(n, N + 1, 2)).astype(np.float64)


def brute(traj, nb, window, g):
    """The rule spelled out for one agent: a python sort of (score, j) over j != g."""
    k0, k1 = window
    key = []
    for j in range(traj.shape[0]):
        if j == g:
            continue
        with np.errstate(invalid="ignore"):
            d = traj[j, k0:k1 + 1] - traj[g, k0:k1 + 1]
            s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).min()
        key.append((np.inf if np.isnan(s) else s, j))
    key.sort()
    return [j for _, j in key[:nb]], [s for s, _ in key[:nb]]


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_window_00_is_nearest_neighbours_on_the_bench_scenario(nb):
    sc = S.make_di(256, 10, nb)
    assert np.array_equal(S.select_neighbours(sc.traj, nb), sc.nbr)
    assert np.array_equal(S.select_neighbours(sc.traj, nb), S.nearest_neighbours(sc.x0[:, :2], nb))
    rows = slice(64, 96)
    assert np.array_equal(S.select_neighbours(sc.traj, nb, rows=rows), sc.nbr[rows])


def test_closest_approach_window_is_a_different_table():
    sc = S.make_di(256, 10, 2)
    far = S.select_neighbours(sc.traj, 2, window=(0, 10))
    assert (far != sc.nbr).any(axis=1).mean() > 0.05
    assert np.array_equal(S.select_neighbours(sc.traj, 2, window=(10, 10)),
                          S.nearest_neighbours(sc.traj[:, 10], 2))


@pytest.mark.parametrize("window", [(0, 0), (0, 2), (1, 2)])
@pytest.mark.parametrize("nb", [1, 3, 12, 64])
def test_ties_break_by_index_and_self_is_left_out_by_index(nb, window):
    t = lattice()
    idx, d2 = S.select_neighbours(t, nb, window, return_dist2=True)
    assert idx.dtype == np.int32 and idx.shape == (65, nb)
    for g in range(65):
        bj, bs = brute(t, nb, window, g)
        assert idx[g].tolist() == bj and d2[g].tolist() == bs
        assert g not in idx[g]
    assert (d2 == 0).any()    # agents on the own agent's point are valid neighbours


def test_all_agents_on_one_point():
    t = np.full((9, 4, 2), 0.25)
    idx = S.select_neighbours(t, 3, (0, 3))
    for g in range(9):
        assert idx[g].tolist() == [j for j in range(9) if j != g][:3]


def test_nan_and_inf_rules():
    rng = np.random.default_rng(5)
    t = rng.normal(size=(13, 6, 2))
    t[4, 2, 0] = np.nan      # inside the window (1, 3): agent 4's score is +inf for everyone
    t[7, 5, 1] = np.nan      # outside it: must not matter
    t[9, 1] = np.inf         # dx = inf at stage 1, finite elsewhere
    t[10, :, 0] = -np.inf
    clean = t.copy()
    clean[7, 5, 1] = 0.0
    idx, d2 = S.select_neighbours(t, 12, (1, 3), return_dist2=True)
    assert np.array_equal(idx, S.select_neighbours(clean, 12, (1, 3)))
    for g in range(13):
        bj, bs = brute(t, 12, (1, 3), g)
        assert idx[g].tolist() == bj and d2[g].tolist() == bs
    assert not np.isnan(d2).any()
    # the own agent NaN: every score +inf, so the lowest indices other than itself
    assert idx[4].tolist() == [j for j in range(13) if j != 4]
    assert np.isinf(d2[4]).all()
    # agent 4 comes last for everyone else, behind the agents at infinity of equal score only by index
    for g in (0, 1, 2, 3):
        assert np.isinf(d2[g, -1]) and 4 in idx[g, -2:]


def test_arguments():
    t = lattice(5, 2)
    assert S.select_neighbours(t, 0).shape == (5, 0)
    for bad in (dict(nb=5), dict(nb=-1), dict(nb=1, window=(2, 1)), dict(nb=1, window=(0, 3)),
                dict(nb=1, window=(-1, 0))):
        with pytest.raises(ValueError):
            S.select_neighbours(t, **bad)
