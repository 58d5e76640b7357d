"""The device neighbour selection (cmpc_nbr_select_dev, csrc/nbr_select.hip) against its numpy statement
`scenarios.select_neighbours`: indices equal, scores equal bit for bit — the rule (min over the window of the
squared distance, NaN as +inf, order by (score, index), the agent itself left out by index) determines the
result completely, ties and non-finite coordinates included.

Sizes one past each boundary of the kernel as written: 128 candidates per tile (kSelTile: n_total 129), 64
lanes (n_total 65), 4 agents per workgroup (batch 5) below 2048 local agents and 8 from there on (kSelWideBatch:
batch 2047, 2048, 2049), 16 stages per LDS chunk (kSelChunk: windows
of 16 and 17 stages), a step of 16 / W tiles for a window of W <= 16 stages (W = 1: 2048 candidates, n_total
2049; W = 2: 1025; W = 3: 641; W = 5: 385; W = 8: 257), per-lane list lengths 2 / 4 / 12 (nb 3, 5)."""
import ctypes as ct

import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S

pytestmark = pytest.mark.gpu

N_TOTALS = [2, 3, 13, 64, 65, 128, 129, 257, 1025]
NBS = [1, 2, 3, 5, 12]


def population(n, N, seed=11):
    """n agents with random positions and velocities, rolled out N stages (paths cross inside the horizon)."""
    rng = np.random.default_rng(seed + 1000 * n + N)
    p = rng.uniform(0.0, 4.0, size=(n, 1, 2))
    v = rng.uniform(-1.0, 1.0, size=(n, 1, 2))
    return np.ascontiguousarray(p + v * np.arange(N + 1)[None, :, None] * 0.1)


def lattice(n=65, N=9, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, size=(n, N + 1, 2)).astype(np.float64)


def windows(N):
    return sorted({(0, 0), (N, N), (0, N)} | ({(3, 7)} if N >= 7 else set()))


def select(ctx, traj, nb, window=(0, 0), batch=None, off=0, with_d2=True):
    import torch

    from cmpc.rounds import select_neighbours_dev

    t = torch.as_tensor(np.ascontiguousarray(traj), dtype=torch.float64, device="cuda")
    B = traj.shape[0] - off if batch is None else batch
    d2 = torch.full((B, nb), -1.0, dtype=torch.float64, device="cuda") if with_d2 else None
    out = select_neighbours_dev(t, nb, batch, off, window, dist2=d2, ctx=ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (d2.cpu().numpy() if with_d2 else None)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check(ctx, traj, nbs, window, batch=None, off=0):
    """Every nb of `nbs` on the device against one host selection of the longest list (a shorter list is
    its prefix: the order is total)."""
    n = traj.shape[0]
    rows = slice(off, n if batch is None else off + batch)
    ref, rd2 = S.select_neighbours(traj, max(nbs), window, rows=rows, return_dist2=True)
    for nb in nbs:
        idx, d2 = select(ctx, traj, nb, window, batch, off)
        assert idx.dtype == np.int32 and np.array_equal(idx, ref[:, :nb]), (n, nb, window)
        assert np.array_equal(bits(d2), bits(rd2[:, :nb])), (n, nb, window)
        assert not (idx == np.arange(n)[rows, None]).any()


@pytest.mark.parametrize("n", N_TOTALS)
def test_matches_host_selection(gpu_ctx, n):
    """n_total x nb in {1, 2, 3, 5, 12, n_total - 1 (a full sort of everyone else)} x N in {1, 9, 30} x the
    windows (0, 0), (N, N), (0, N), (3, 7)."""
    for N in (1, 9, 30) if n <= 257 else (30,):
        t = population(n, N)
        nbs = sorted({nb for nb in NBS if nb < n} | ({n - 1} if n - 1 <= 12 else set()))
        for w in windows(N):
            check(gpu_ctx, t, nbs, w)


@pytest.mark.parametrize("window", [(3, 18), (3, 19), (0, 15), (0, 16), (14, 30)])
def test_window_chunk_boundaries(gpu_ctx, window):
    check(gpu_ctx, population(129, 30), [2, 12], window)


@pytest.mark.parametrize("n,window", [(2048, (0, 0)), (2049, (9, 9)), (1025, (0, 1)), (641, (4, 6)), (385, (3, 7)),
                                      (257, (2, 9)), (384, (3, 7))])
def test_step_boundaries(gpu_ctx, n, window):
    """One past (and exactly) the candidates one step stages for a short window."""
    check(gpu_ctx, population(n, 9), [2, 5], window)
    check(gpu_ctx, population(n, 9), [3], window, 5, n - 5)


def test_eight_agents_per_workgroup(gpu_ctx):
    """From 2048 local agents on a workgroup holds 8: both sides of the threshold on one population (a batch
    that is no multiple of 8, every list length), and a two-chunk window on the wide path."""
    t = population(2049, 9)
    check(gpu_ctx, t, [2], (0, 0), 2047, 2)
    check(gpu_ctx, t, [2, 3, 12], (0, 0))
    check(gpu_ctx, t, [5], (3, 7), 2048, 1)
    check(gpu_ctx, population(2049, 30), [2, 12], (3, 19))


def test_long_horizon(gpu_ctx):
    """N = 125 (the reference's horizon): 126 stages, eight chunks."""
    check(gpu_ctx, population(70, 125), [3], (0, 125))
    check(gpu_ctx, population(70, 125), [3], (125, 125))


@pytest.mark.parametrize("n,batch,off", [(96, 32, 64), (96, 32, 0), (96, 32, 32), (129, 5, 124), (13, 1, 12)])
def test_shards(gpu_ctx, n, batch, off):
    for w in ((0, 0), (0, 9)):
        check(gpu_ctx, population(n, 9), [2, 5], w, batch, off)


def test_three_shards_equal_the_unsharded_call(gpu_ctx):
    t = population(96, 9)
    for w in ((0, 0), (0, 9), (3, 7)):
        full, fd2 = select(gpu_ctx, t, 3, w)
        parts = [select(gpu_ctx, t, 3, w, 32, off) for off in (0, 32, 64)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), full)
        assert np.array_equal(bits(np.concatenate([p[1] for p in parts])), bits(fd2))


@pytest.mark.parametrize("window", [(0, 0), (0, 9), (3, 7)])
def test_ties_on_the_lattice(gpu_ctx, window):
    """65 agents on {0..3}^2: exact zero and equal scores, agents on the own agent's point."""
    t = lattice()
    check(gpu_ctx, t, [1, 2, 3, 12], window)
    check(gpu_ctx, t, [12], window, 32, 33)
    assert (S.select_neighbours(t, 12, window, return_dist2=True)[1] == 0).any()


def test_all_agents_on_one_point(gpu_ctx):
    for n, nb in ((13, 12), (65, 3), (130, 12)):
        t = np.full((n, 4, 2), 0.25)
        idx, d2 = select(gpu_ctx, t, nb, (0, 3))
        for g in range(n):
            assert idx[g].tolist() == [j for j in range(n) if j != g][:nb]
        assert (d2 == 0).all()


def test_non_finite_inputs(gpu_ctx):
    t = population(70, 9)
    t[4, 5, 0] = np.nan        # a candidate NaN inside the window (3, 7)
    t[7, 9, 1] = np.nan        # ... and one NaN outside it
    t[9, 4] = np.inf
    t[10, :, 0] = -np.inf
    t[66, :, :] = np.inf
    t[20, 3:8] = np.nan        # an own agent that is NaN
    clean = t.copy()
    clean[7, 9, 1] = 0.0
    for nb in (2, 12):
        check(gpu_ctx, t, [nb], (3, 7))
        a, ad = select(gpu_ctx, t, nb, (3, 7))
        b, bd = select(gpu_ctx, clean, nb, (3, 7))
        assert np.array_equal(a, b) and np.array_equal(bits(ad), bits(bd))   # NaN outside the window: no effect
        assert a[20].tolist() == [j for j in range(70) if j != 20][:nb] and np.isinf(ad[20]).all()
        assert not np.isnan(ad).any()
    check(gpu_ctx, t, [12], (0, 9))    # every NaN inside
    t13 = population(13, 9)
    t13[3, 0] = np.nan
    t13[5, 0, 1] = -np.inf
    check(gpu_ctx, t13, [12], (0, 0))  # the full sort with +inf scores: order by index among them


def test_deterministic_and_dist2_optional(gpu_ctx):
    t = lattice(129, 9, seed=8)
    a, ad = select(gpu_ctx, t, 5, (0, 9))
    b, bd = select(gpu_ctx, t, 5, (0, 9))
    c, _ = select(gpu_ctx, t, 5, (0, 9), with_d2=False)
    assert np.array_equal(a, b) and np.array_equal(bits(ad), bits(bd)) and np.array_equal(a, c)


def _call(ctx, t, nbr, d2, **kw):
    """The C entry point itself on a 13-agent, N = 9 buffer (any pointer may be None), valid unless `kw` says so."""
    d = dict(batch=13, N=9, nb=2, self_offset=0, n_total=13, k0=0, k1=0)
    d.update(kw)
    dims = L.cmpc_nbr_dims(*(d[k] for k in ("batch", "N", "nb", "self_offset", "n_total", "k0", "k1")))
    p = lambda x, ty: None if x is None else ct.cast(ct.c_void_p(x.data_ptr()), ty)  # noqa: E731
    return ctx.lib.cmpc_nbr_select_dev(ctx.h, ct.byref(dims), p(t, L._DP), p(nbr, L._IP), p(d2, L._DP), None)


def test_argument_errors_and_empty_calls(gpu_ctx):
    import torch

    t = torch.as_tensor(population(13, 9), device="cuda")
    nbr = torch.full((13, 12), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((13, 12), -7.0, dtype=torch.float64, device="cuda")
    lib, E = gpu_ctx.lib, L.CMPC_ERR_ARG
    assert lib.cmpc_nbr_select_dev(gpu_ctx.h, None, ct.cast(ct.c_void_p(t.data_ptr()), L._DP),
                                   ct.cast(ct.c_void_p(nbr.data_ptr()), L._IP), None, None) == E
    assert _call(gpu_ctx, None, nbr, d2) == E
    assert _call(gpu_ctx, t, None, d2) == E
    for bad in (dict(nb=-1), dict(nb=13), dict(nb=13, n_total=14, batch=13), dict(nb=12, n_total=12, batch=12),
                dict(self_offset=-1), dict(self_offset=1), dict(batch=14), dict(batch=3, self_offset=11),
                dict(batch=-1), dict(N=0), dict(k0=-1), dict(k0=1, k1=0), dict(k1=10), dict(k0=10, k1=10)):
        assert _call(gpu_ctx, t, nbr, d2, **bad) == E, bad
        assert gpu_ctx.lib.cmpc_last_error(gpu_ctx.h)
    # nothing to select: OK without a launch (null outputs are fine then), outputs untouched
    assert _call(gpu_ctx, t, nbr, d2, batch=0) == L.CMPC_OK
    assert _call(gpu_ctx, t, nbr, d2, nb=0) == L.CMPC_OK
    assert _call(gpu_ctx, t, None, None, nb=0) == L.CMPC_OK
    assert _call(gpu_ctx, t, None, None, batch=0, self_offset=13) == L.CMPC_OK
    torch.cuda.synchronize()
    assert (nbr == -7).all() and (d2 == -7.0).all()
    # and the largest valid call still runs: nb = 12 = n_total - 1, the last window
    assert _call(gpu_ctx, t, nbr, d2, nb=12, k0=9, k1=9) == L.CMPC_OK
    torch.cuda.synchronize()
    assert np.array_equal(nbr.cpu().numpy(), S.select_neighbours(t.cpu().numpy(), 12, (9, 9)))
