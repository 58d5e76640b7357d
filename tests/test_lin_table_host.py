"""The stage-table rule of the linear-model rounds on the host (cmpc.scenarios.lin_table_rows / lin_window /
lin_table_of_di): the index vector against a literal loop, the window against fancy indexing, the double integrator
as the one-row table, and the argument errors.  No GPU."""
import numpy as np
import pytest

from cmpc import scenarios as S

HOLD, PERIODIC = S.TABLE_HOLD, S.TABLE_PERIODIC


def rows_loop(T, t, n, mode):
    out = []
    for k in range(n):
        tau = t + k
        out.append(tau % T if mode == PERIODIC else min(tau, T - 1))
    return out


@pytest.mark.parametrize("mode", [HOLD, PERIODIC])
@pytest.mark.parametrize("T,n", [(1, 1), (1, 7), (6, 4), (3, 11), (7, 11), (14, 11), (75, 71)])
def test_table_rows_equal_the_literal_loop(T, n, mode):
    # t = 0, inside, the last rows (near the end), the end itself and far past it
    for t in sorted({0, 1, max(T - n, 0), max(T - 2, 0), T - 1, T, 2 * T + 1, 1000}):
        r = S.lin_table_rows(T, t, n, mode)
        assert r.dtype == np.int64 and r.shape == (n,)
        assert r.tolist() == rows_loop(T, t, n, mode), (T, t, n, mode)
        assert ((0 <= r) & (r < T)).all()
    assert S.lin_table_rows(T, 3, 0, mode).shape == (0,)


def test_table_rows_wrap_and_hold():
    assert S.lin_table_rows(3, 2, 11, PERIODIC).tolist() == [2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0]     # wraps three times
    assert S.lin_table_rows(6, 4, 4, HOLD).tolist() == [4, 5, 5, 5]                                # straddles the end
    assert S.lin_table_rows(6, 9, 4, HOLD).tolist() == [5, 5, 5, 5]                                # wholly past it
    assert S.lin_table_rows(6, 4, 4).tolist() == [4, 5, 5, 5]                                      # HOLD is the default


def random_table(n, T, nx, nu, mo, seed=5):
    rng = np.random.default_rng(seed)
    return dict(A=rng.standard_normal((n, T, nx, nx)), B=rng.standard_normal((n, T, nx, nu)),
                qlin=rng.standard_normal((n, T, nx)), C=rng.standard_normal((n, T, mo, nx)) if mo else None,
                h=rng.standard_normal((n, T, mo)) if mo else None)


@pytest.mark.parametrize("n,T,nx,nu,mo,N,mode,t", [(3, 6, 4, 2, 4, 3, HOLD, 0), (3, 6, 4, 2, 4, 3, HOLD, 4),
                                                   (3, 6, 4, 2, 4, 3, HOLD, 9), (2, 3, 9, 2, 4, 10, PERIODIC, 2),
                                                   (1, 1, 12, 4, 0, 1, HOLD, 0), (2, 5, 6, 3, 2, 4, PERIODIC, 4)])
def test_window_equals_fancy_indexing(n, T, nx, nu, mo, N, mode, t):
    tab = random_table(n, T, nx, nu, mo)
    tab["qlin"][0, 0, 0] = -0.0
    tab["A"][0, T - 1, 0, 0] = np.nan                       # copies: a NaN and a negative zero travel as they are
    A, B, own = S.lin_window(tab, t, N, mode)
    r = np.array(rows_loop(T, t, N + 1, mode))
    assert A.shape == (n, N, nx, nx) and B.shape == (n, N, nx, nu) and own["qlin_own"].shape == (n, N + 1, nx)
    assert A.tobytes() == tab["A"][:, r[:N]].tobytes() and B.tobytes() == tab["B"][:, r[:N]].tobytes()
    assert own["qlin_own"].tobytes() == tab["qlin"][:, r].tobytes()
    if mo:
        assert own["C_own"].shape == (n, N, mo, nx) and own["h_own"].shape == (n, N, mo)
        assert own["C_own"].tobytes() == tab["C"][:, r[1:]].tobytes()
        assert own["h_own"].tobytes() == tab["h"][:, r[1:]].tobytes()
    else:
        assert own["C_own"] is None and own["h_own"] is None
    # the window is a copy: writing it leaves the table alone
    before = tab["qlin"].copy()
    own["qlin_own"][:] = 7.0
    assert tab["qlin"].tobytes() == before.tobytes()
    # and it is lin_rows' input as it stands
    traj = np.random.default_rng(1).standard_normal((n, N + 1, 2))
    q, C, h = S.lin_rows(dict(ix=0, iy=1, min_dist=0.25, wq=5.0), own, np.zeros((n, 0), np.int32), traj)
    assert q.shape == (n, N + 1, nx) and C.shape == (n, N, mo, nx) and h.shape == (n, N, mo)


@pytest.mark.parametrize("dim", [2, 3])
def test_double_integrator_is_the_one_row_table(dim):
    sc = S.make_di(8, 6, 2, dim)
    lin = S.lin_of_di(sc)
    for T in (1, 4):
        tl = S.lin_table_of_di(sc, T)
        assert tl["mode"] == HOLD and S.lin_table_rows_of(tl["table"]) == T
        assert tl["prm"] == lin["prm"] and np.array_equal(tl["nbr"], lin["nbr"]) and tl["self_offset"] == 0
        for t in (0, 1, 5, 1000):
            A, B, own = S.lin_window(tl["table"], t, sc.N, tl["mode"])
            assert A.tobytes() == np.ascontiguousarray(sc.A, np.float64).tobytes()
            assert B.tobytes() == np.ascontiguousarray(sc.B, np.float64).tobytes()
            for k in ("qlin_own", "C_own", "h_own"):
                assert own[k].shape == lin["own"][k].shape and own[k].tobytes() == lin["own"][k].tobytes(), (T, t, k)
    half = S.lin_table_of_di(sc, 1, rows=slice(4, 8))
    assert half["self_offset"] == 4 and half["table"]["A"].shape[0] == 4
    assert half["table"]["h"].tobytes() == S.lin_of_di(sc, slice(4, 8))["own"]["h_own"][:, :1].tobytes()


def test_bad_arguments_raise():
    for args in ((0, 0, 3, HOLD), (-1, 0, 3, HOLD), (4, -1, 3, HOLD), (4, 0, -1, HOLD), (4, 0, 3, 2), (4, 0, 3, -1)):
        with pytest.raises(ValueError):
            S.lin_table_rows(*args)
    tab = random_table(2, 5, 4, 2, 3)
    for bad in (dict(tab, A=tab["A"][:, :4]), dict(tab, B=tab["B"][:1]), dict(tab, qlin=tab["qlin"][:, :, :3]),
                dict(tab, C=tab["C"][:, :4]), dict(tab, h=tab["h"][:, :, :2]), dict(tab, h=None),
                dict(tab, A=tab["A"][:, :, 0])):
        with pytest.raises(ValueError):
            S.lin_window(bad, 0, 3)
    for t, N, mode in ((-1, 3, HOLD), (0, 0, HOLD), (0, 3, 5)):
        with pytest.raises(ValueError):
            S.lin_window(tab, t, N, mode)
    sc = S.make_di(4, 5, 2, 2)
    with pytest.raises(ValueError):
        S.lin_table_of_di(sc, 0)
    sc.A[1, 2, 0, 0] += 1.0                                 # a time-varying "double integrator" is no one-row table
    with pytest.raises(ValueError):
        S.lin_table_of_di(sc)
