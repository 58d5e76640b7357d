"""The linear-model round family without a GPU: the numpy statements of its builder and advance
(cmpc.scenarios.lin_rows / lin_advance, the rule of cmpc_lin_build_dev / cmpc_lin_advance_dev in include/cmpc.h)
against the oracle's double-integrator builder, their edge cases, and the symbols libcmpc.so exports."""
import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S


@pytest.mark.parametrize("dim", [2, 3])
def test_lin_rows_of_the_double_integrator_equal_the_oracle(dim):
    """lin_rows on lin_of_di is the oracle's builder: the own rows, the plane coefficients and the cost bit for
    bit (they go through the same elementwise operations); the planes' right-hand sides within 2 ulp of the
    terms they are summed from (the oracle forms bb with v @ (pe + pn), a dot product that may round differently
    from the written-out sum)."""
    from oracle import synth

    sc = S.make_di(12, 6, nb=2, dim=dim)
    P = synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj, np.arange(12))
    lin = S.lin_of_di(sc)
    assert (lin["prm"]["ix"], lin["prm"]["iy"]) == (0, 1) and lin["own"]["C_own"].shape[2] == 4
    assert lin["prm"]["min_dist"] == sc.params["min_dist"] and lin["prm"]["wq"] == sc.params["wq"]
    q_own = lin["own"]["qlin_own"]
    other = [c for c in range(2 * dim) if c not in (1, dim)]
    assert not q_own[:, :, other].view(np.uint64).any()          # exact +0.0 elsewhere
    qlin, C, h = S.lin_rows(**lin)
    assert C.tobytes() == P["C"].tobytes()
    assert qlin.tobytes() == P["qlin"].tobytes()
    assert h[..., :4].tobytes() == P["h"][..., :4].tobytes()
    # h = -d/2 - bb, bb = -0.5 (t1 + t2) with t1 = ax (ex + nx), t2 = ay (ey + ny) of opposite signs here: the two
    # roundings of t1 + t2 differ by an ulp of the TERMS, which the cancellation leaves as several ulps of the small
    # result (measured: 4 ulp of h, 1 ulp of the terms).  The 2 ulp are therefore taken at the largest magnitude
    # that was rounded on the way: max(|t1|, |t2|, |h|)
    me, C4 = sc.traj[:, :-1], C[:, :, 4:]
    scale = np.abs(h[..., 4:])
    for i in range(2):
        s = me + sc.traj[sc.nbr[:, i], :-1]
        scale[..., i] = np.maximum(scale[..., i], np.maximum(np.abs(C4[:, :, i, 0] * s[..., 0]),
                                                             np.abs(C4[:, :, i, 1] * s[..., 1])))
    assert np.isfinite(h).all() and (np.abs(h[..., 4:] - P["h"][..., 4:]) <= 2 * np.spacing(scale)).all()


def small_instance(rng, nx, mo, nb, N, B, n_total=None):
    n = n_total or B + 2
    own = dict(qlin_own=rng.standard_normal((B, N + 1, nx)), C_own=rng.standard_normal((B, N, mo, nx)),
               h_own=rng.standard_normal((B, N, mo)))
    traj = rng.standard_normal((n, N + 1, 2))
    nbr = np.stack([rng.permutation([j for j in range(n) if j != b])[:nb] for b in range(B)]).astype(np.int32) \
        if nb else np.zeros((B, 0), np.int32)
    return own, nbr, traj


def test_lin_rows_edge_cases():
    rng = np.random.default_rng(5)
    # no neighbours: the own rows and the own cost (the coverage term adds the 0.0 it accumulated)
    own, nbr, traj = small_instance(rng, 6, 2, 0, 4, 2)
    q, C, h = S.lin_rows(dict(ix=0, iy=1, min_dist=0.25, wq=5.0), own, nbr, traj)
    assert np.array_equal(q, own["qlin_own"]) and np.array_equal(C, own["C_own"]) and np.array_equal(h, own["h_own"])
    # no own rows (None and empty arrays alike): only the planes, on columns iy < ix
    own, nbr, traj = small_instance(rng, 12, 0, 1, 1, 1)
    prm = dict(ix=11, iy=0, min_dist=0.25, wq=5.0)
    q, C, h = S.lin_rows(prm, own, nbr, traj)
    q2, C2, h2 = S.lin_rows(prm, dict(qlin_own=own["qlin_own"], C_own=None, h_own=None), nbr, traj)
    assert C.shape == (1, 1, 1, 12) and h.shape == (1, 1, 1)
    assert q.tobytes() == q2.tobytes() and C.tobytes() == C2.tobytes() and h.tobytes() == h2.tobytes()
    d = traj[nbr[0, 0], 0] - traj[0, 0]
    a = d / np.sqrt(d[0] * d[0] + d[1] * d[1])
    assert C[0, 0, 0, 11] == a[0] and C[0, 0, 0, 0] == a[1] and not C[0, 0, 0, 1:11].any()
    assert np.array_equal(q[0, 0], own["qlin_own"][0, 0])        # stage 0: no coverage term
    # the local agents are rows self_offset.. of traj; a neighbour on the agent's own point: NaN, that agent only
    own, nbr, traj = small_instance(rng, 4, 4, 2, 3, 2, n_total=5)
    nbr[:] = [[0, 1], [0, 4]]
    traj[4, 1] = traj[3, 1]                                      # agent 1 (global 3) and neighbour 4 at stage 1
    q, C, h = S.lin_rows(dict(ix=2, iy=3, min_dist=0.25, wq=5.0), own, nbr, traj, self_offset=2)
    assert np.isfinite(q[0]).all() and np.isfinite(C[0]).all() and np.isfinite(h[0]).all()
    assert np.isnan(C[1, 1, 5, 2:]).all() and np.isnan(h[1, 1, 5]) and np.isnan(q[1, 2, 2:]).all()
    assert np.isfinite(C[1, 0]).all() and np.isfinite(C[1, 2]).all() and np.isfinite(q[1, 1]).all()
    for bad in (dict(ix=1, iy=1), dict(ix=-1, iy=0), dict(ix=0, iy=4)):
        with pytest.raises(ValueError):
            S.lin_rows(dict(min_dist=0.25, wq=5.0, **bad), own, nbr, traj)


def test_lin_advance_skips_a_non_finite_agent():
    rng = np.random.default_rng(6)
    nx, nu, ns, N, B = 5, 2, 1, 3, 4
    nxe = nx + ns
    z = rng.standard_normal((B, nxe * (N + 1) + 2 * nu * N))
    z[2, -1] = np.nan                                            # in the du block, which the advance never copies
    z[3, 7] = np.inf
    x0, up, tr = rng.standard_normal((B, nx)), rng.standard_normal((B, nu)), rng.standard_normal((B, N + 1, 2))
    keep = (x0.copy(), up.copy(), tr.copy())
    x1, u1, t1 = S.lin_advance(dict(ix=4, iy=1), z, nx, nu, ns, N, x0, up, tr)
    assert all(np.array_equal(a, b) for a, b in zip((x0, up, tr), keep))          # the arguments are left alone
    for b in (0, 1):
        assert np.array_equal(x1[b], z[b, nxe:nxe + nx]) and np.array_equal(u1[b], z[b, nxe * (N + 1):][:nu])
        for k in range(N + 1):
            assert t1[b, k, 0] == z[b, k * nxe + 4] and t1[b, k, 1] == z[b, k * nxe + 1]
    for b in (2, 3):
        assert np.array_equal(x1[b], x0[b]) and np.array_equal(u1[b], up[b]) and np.array_equal(t1[b], tr[b])
    with pytest.raises(ValueError):
        S.lin_advance(dict(ix=4, iy=1), z[:, :-1], nx, nu, ns, N, x0, up, tr)


def test_library_exports_the_family():
    lib = L.load()
    names = ["cmpc_lin_build_dev", "cmpc_lin_advance_dev", "cmpc_lin_round_dev"] + \
        ["cmpc_lin_rounds_" + k for k in ("create", "step", "read", "history", "get_traj", "set_traj", "set_state",
                                          "destroy", "log_enable", "log_range", "log_read")]
    for name in names:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.cmpc_abi_version() == 6
