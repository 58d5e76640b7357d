"""3-D positions on the linear-model family without a GPU: the numpy statements with ``iz`` in prm
(cmpc.scenarios.lin_rows / lin_advance / lin_publish / select_neighbours, the rules of cmpc_lin3_* and
cmpc_nbr_select3_dev in include/cmpc.h), the stacked population, and the library's exports."""
import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S
from lin3_cases import (PRM, PUBLISH_SHAPE, brute_select, build_instance, planted, population, positions,
                        publish_instance)


def test_coplanar_rows_are_the_planar_rows():
    """One third coordinate for everybody: dz = 0 adds an exact zero to every sum, so qlin, C, h are lin_rows' planar
    ones byte for byte, and the iz column of the plane rows is zero."""
    sc = S.make_di(16, 6, 2, 3)
    lin = S.lin_of_di(sc)
    want = S.lin_rows(**lin)
    for alt in (0.0, 1.75):
        l3 = S.lin3_of_di(sc, alt)
        assert l3["prm"]["iz"] == 2 and l3["traj"].shape == (16, 7, 3) and (l3["traj"][..., 2] == alt).all()
        assert np.array_equal(l3["traj"][..., :2], sc.traj) and (l3["x0"][:, 2] == alt).all()
        got = S.lin_rows(l3["prm"], l3["own"], l3["nbr"], l3["traj"], l3["self_offset"])
        for name, g, w in zip(("qlin", "C", "h"), got, want):
            assert np.isfinite(w).all() and np.array_equal(g, w), (alt, name)
        assert not got[1][:, :, 4:, 2].any()
    with pytest.raises(ValueError):
        S.lin3_of_di(S.make_di(6, 4, 2, 2), 0.0)


def test_coincidence_is_three_dimensional():
    shape = (6, 4, 2, 3, 2, 0, 1, 2)
    prm, own, nbr, traj, off = build_instance(shape, 5)
    nbr[:] = [[0, 4], [0, 3]]
    traj[3, 1, :2] = traj[off + 1, 1, :2]                # agent 1's neighbour 3 over its ground point at stage 1 ..
    q, C, h = S.lin_rows(prm, own, nbr, traj, off)
    assert all(np.isfinite(a).all() for a in (q, C, h))  # .. at another altitude: finite
    assert C[1, 1, 5, 0] == 0.0 and C[1, 1, 5, 1] == 0.0 and abs(C[1, 1, 5, 2]) == 1.0   # the normal is vertical
    planar = S.lin_rows(dict(PRM, ix=0, iy=1), own, nbr, traj[..., :2].copy(), off)
    assert np.isnan(planar[1][1, 1, 5, :2]).all()        # the planar rule has no plane there
    traj[3, 1, 2] = traj[off + 1, 1, 2]                  # on its 3-D point: NaN, that agent and stage only
    q, C, h = S.lin_rows(prm, own, nbr, traj, off)
    assert np.isnan(C[1, 1, 5, :3]).all() and np.isnan(h[1, 1, 5]) and np.isnan(q[1, 2, :3]).all()
    assert np.isnan(C).sum() == 3 and np.isnan(h).sum() == 1 and np.isnan(q).sum() == 3
    assert all(np.isfinite(a[0]).all() for a in (q, C, h))


def test_rows_written_out():
    """One agent, one neighbour, one stage, position columns in any order: the header's expressions one by one."""
    shape = (12, 0, 1, 1, 1, 11, 0, 5)
    prm, own, nbr, traj, off = build_instance(shape)
    q, C, h = S.lin_rows(prm, own, nbr, traj, off)
    e, n = traj[off, 0], traj[nbr[0, 0], 0]
    dx, dy, dz = n - e
    nrm = np.sqrt(dx * dx + dy * dy + dz * dz)
    ax, ay, az = dx / nrm, dy / nrm, dz / nrm
    bb = -0.5 * (ax * (e[0] + n[0]) + ay * (e[1] + n[1]) + az * (e[2] + n[2]))
    assert (C[0, 0, 0, 11], C[0, 0, 0, 0], C[0, 0, 0, 5]) == (ax, ay, az) and h[0, 0, 0] == -0.25 / 2 - bb
    assert not C[0, 0, 0, [1, 2, 3, 4, 6, 7, 8, 9, 10]].any()
    qx, qy, qz = traj[off, 1] - traj[nbr[0, 0], 1]
    wgt = (2.0 * 0.25 - np.sqrt(qx * qx + qy * qy + qz * qz)) / 1
    qo = own["qlin_own"]
    assert q[0, 1, 11] == qo[0, 1, 11] + (0.0 + 5.0 * wgt * ax) and q[0, 1, 0] == qo[0, 1, 0] + (0.0 + 5.0 * wgt * ay)
    assert q[0, 1, 5] == qo[0, 1, 5] + (0.0 + 5.0 * wgt * az)
    assert np.array_equal(q[0, 0], qo[0, 0])             # stage 0: no coverage term
    # no own rows given as None; no neighbours: the copies alone
    q2, C2, h2 = S.lin_rows(prm, dict(qlin_own=qo, C_own=None, h_own=None), nbr, traj, off)
    assert q.tobytes() == q2.tobytes() and C.tobytes() == C2.tobytes() and h.tobytes() == h2.tobytes()
    prm, own, nbr, traj, off = build_instance((6, 2, 0, 4, 2, 0, 1, 2))
    q, C, h = S.lin_rows(prm, own, nbr, traj, off)
    assert np.array_equal(q, own["qlin_own"]) and np.array_equal(C, own["C_own"]) and np.array_equal(h, own["h_own"])


@pytest.mark.parametrize("window", [(0, 0), (0, 6), (2, 4)])
def test_select_neighbours_against_a_brute_force_loop(window):
    traj = planted(population(23, 6))
    rows = np.arange(23)
    for nb in (1, 2, 5):
        nbr, d2 = S.select_neighbours(traj, nb, window, return_dist2=True)
        wn, wd = brute_select(traj, nb, window, rows)
        assert nbr.dtype == np.int32 and np.array_equal(nbr, wn) and d2.tobytes() == wd.tobytes(), (nb, window)
    nbr, d2 = S.select_neighbours(traj, 3, window, return_dist2=True)
    assert list(nbr[1, :2]) == [11, 22] and (d2[1, :2] == 0.0).all()         # equal scores: the index decides
    assert nbr[2, 0] == 3 and nbr[3, 0] == 2 and d2[2, 0] == 0.0
    if window[1] == 6:                                                       # the NaN is in the window
        full = S.select_neighbours(traj, 22, window)
        assert (full[np.arange(23) != 5, -1] == 5).all()                     # everybody's last choice
        assert np.isinf(S.select_neighbours(traj, 2, window, rows=slice(5, 6), return_dist2=True)[1]).all()
    # the third coordinate decides: two agents over one ground point are not each other's nearest when a third
    # agent is closer in space
    t = np.zeros((3, 1, 3))
    t[1, 0] = (0.0, 0.0, 2.0)
    t[2, 0] = (1.0, 0.0, 0.0)
    assert S.select_neighbours(t, 1)[0, 0] == 2 and S.select_neighbours(t[..., :2].copy(), 1)[0, 0] == 1
    # a sharded call
    part = S.select_neighbours(traj, 2, window, rows=slice(7, 12))
    assert np.array_equal(part, S.select_neighbours(traj, 2, window)[7:12])


def test_publish_and_advance_edge_cases():
    shape = PUBLISH_SHAPE
    nx, ns, nu, N, B, ix, iy, iz, n, off = shape
    prm, z, traj, _ = publish_instance()
    z0, traj0 = z.copy(), traj.copy()
    tl, close, delta, not_close = S.lin_publish(prm, z, nx, nu, ns, N, traj, self_offset=off)
    assert np.array_equal(z, z0, equal_nan=True) and np.array_equal(traj, traj0, equal_nan=True)
    assert tl.shape == (B, N + 1, 3) and close.dtype == np.int32 and close.shape == delta.shape == (B,)
    new = positions(shape, z)
    for b in (0, 1):                                     # a non-finite z: the row of the exchange buffer again
        assert tl[b].tobytes() == traj[off + b].tobytes() and close[b] == 0 and np.isnan(delta[b])
        assert np.isfinite(new[b]).all()
    assert tl[2].tobytes() == new[2].tobytes() and close[2] == 0 and np.isnan(delta[2])   # a NaN in prev
    assert np.signbit(tl[3, 1, 0]) and np.signbit(tl[3, 2, 1]) and np.signbit(tl[3, 3, 2]) and tl[3, 3, 2] == 0.0
    assert tl[3].tobytes() == new[3].tobytes() and close[3] == 0 and 0.01 < delta[3] <= 0.05
    assert close[4] == 1 and 0.0 < delta[4] <= 0.005 and delta[4] == np.abs(traj[off + 4] - new[4]).max()
    assert close[5] == 0 and not_close == 5
    # the allclose threshold on the third coordinate alone (exact in fp64): |1.0 - 1.25| is close at atol 0.25
    zt = np.random.default_rng(2).standard_normal(z.shape)
    nxe = nx + ns
    for k in range(N + 1):
        zt[:, k * nxe + ix] = zt[:, k * nxe + iy] = zt[:, k * nxe + iz] = 1.25
    zt[1::2, N * nxe + iz] = np.nextafter(1.25, 2.0)
    tt = traj.copy()
    tt[off:off + B] = 1.0
    _, close, delta, cnt = S.lin_publish(prm, zt, nx, nu, ns, N, tt, atol=0.25, rtol=0.0, self_offset=off)
    assert list(close) == [1, 0] * 3 and cnt == 3 and (delta[::2] == 0.25).all() and (delta[1::2] > 0.25).all()
    # the advance: the guard, and three columns
    rng = np.random.default_rng(6)
    x0, up, tr = rng.standard_normal((B, nx)), rng.standard_normal((B, nu)), rng.standard_normal((B, N + 1, 3))
    keep = (x0.copy(), up.copy(), tr.copy())
    x1, u1, t1 = S.lin_advance(prm, z, nx, nu, ns, N, x0, up, tr)
    assert all(np.array_equal(a, b) for a, b in zip((x0, up, tr), keep))
    for b in (0, 1):
        assert np.array_equal(x1[b], x0[b]) and np.array_equal(u1[b], up[b]) and np.array_equal(t1[b], tr[b])
    for b in (2, 3, 4, 5):
        assert np.array_equal(x1[b], z[b, nxe:nxe + nx]) and np.array_equal(u1[b], z[b, nxe * (N + 1):][:nu])
        assert t1[b].tobytes() == new[b].tobytes()


def test_value_errors():
    shape = (6, 4, 2, 3, 2, 0, 1, 2)
    prm, own, nbr, traj, off = build_instance(shape)
    nx, ns, nu, N, B = 6, 1, 3, 3, 2
    z = np.zeros((B, (nx + ns) * (N + 1) + 2 * nu * N))
    x0, up = np.zeros((B, nx)), np.zeros((B, nu))
    for bad in (dict(iz=0), dict(iz=1), dict(iz=6), dict(iz=-1)):
        p = dict(prm, **bad)
        with pytest.raises(ValueError):
            S.lin_rows(p, own, nbr, traj, off)
        with pytest.raises(ValueError):
            S.lin_publish(p, z, nx, nu, ns, N, traj, self_offset=off)
        with pytest.raises(ValueError):
            S.lin_advance(p, z, nx, nu, ns, N, x0, up, traj[off:off + B])
    flat = traj[..., :2].copy()                          # a 2-column buffer with iz set
    with pytest.raises(ValueError):
        S.lin_rows(prm, own, nbr, flat, off)
    with pytest.raises(ValueError):
        S.lin_publish(prm, z, nx, nu, ns, N, flat, self_offset=off)
    with pytest.raises(ValueError):
        S.lin_advance(prm, z, nx, nu, ns, N, x0, up, flat[off:off + B])
    with pytest.raises(ValueError):                      # and a 3-column one without it
        S.lin_rows(dict(PRM, ix=0, iy=1), own, nbr, traj, off)
    with pytest.raises(ValueError):
        S.make_stacked(11, 5)


def test_stacked_population():
    m = S.make_stacked(12, 50)
    sh = m["shared"]
    assert (sh["nx"], sh["nu"], sh["N"], sh["mc"]) == (6, 3, 50, 6) and m["prm"]["iz"] == 2
    x0, traj = m["x0"], m["traj"]
    assert traj.shape == (12, 51, 3) and np.array_equal(traj[:, 0], x0[:, :3])
    assert np.array_equal(x0[1::2, :2], x0[::2, :2]) and np.array_equal(x0[1::2, 3:], x0[::2, 3:])
    assert (x0[::2, 2] == 0.0).all() and (x0[1::2, 2] == 0.6).all()
    assert np.array_equal(m["own"]["qlin_own"][1::2], m["own"]["qlin_own"][::2])          # the lane of the agent below
    assert np.array_equal(m["nbr"], S.select_neighbours(traj, 2)) and (m["nbr"][:, 0] == np.arange(12) ^ 1).all()
    # the planar rule on the first two columns: the partner is on the agent's point at every stage
    q, C, h = S.lin_rows(dict(PRM, ix=0, iy=1), m["own"], m["nbr"], traj[..., :2].copy())
    assert (np.isnan(q).sum(), np.isnan(C).sum(), np.isnan(h).sum()) == (1200, 1200, 600)
    q, C, h = S.lin_rows(m["prm"], m["own"], m["nbr"], traj)
    assert all(np.isfinite(a).all() for a in (q, C, h))
    assert (np.abs(C[:, :, 4, 2]) == 1.0).all() and not C[:, :, 4, :2].any()              # the partner: a vertical normal


def test_library_exports_the_3d_entries():
    lib = L.load()
    names = ["cmpc_lin3_" + k for k in ("build_dev", "table_build_dev", "advance_dev", "publish_dev", "round_dev",
                                        "table_round_dev")] + \
        ["cmpc_nbr_select3_dev", "cmpc_lin_rounds_create3", "cmpc_lin_rounds_create_table3", "cmpc_lin_rounds_pos_dim"]
    for name in names:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.cmpc_abi_version() == 6
    assert ct_size(L.cmpc_lin3_params) == 32


def ct_size(t):
    import ctypes as ct

    return ct.sizeof(t)
