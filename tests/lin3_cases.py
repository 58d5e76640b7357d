"""What the host and the GPU tests of the 3-D positions share (tests/test_lin3_host.py, _gpu.py): the builder's
shapes and instances, the publication's planted agents, the selector's populations and a brute-force selection."""
import numpy as np

PRM = dict(min_dist=0.25, wq=5.0)

# (nx, mo, nb, N, batch, ix, iy, iz): the 3-D double integrator's shape; position columns in any order; no own rows;
# no neighbours (the copies alone); more stages than the workgroup has lanes
BUILD_SHAPES = [(6, 4, 2, 3, 5, 0, 1, 2), (9, 4, 3, 2, 3, 7, 8, 2), (12, 0, 1, 1, 1, 11, 0, 5), (6, 2, 0, 4, 2, 0, 1, 2),
                (6, 4, 2, 70, 2, 0, 1, 2)]


def same(a, b):
    """Finite entries bit for bit, NaNs in the same places (their payloads differ between host and device)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and \
        np.where(nan, 0.0, a).tobytes() == np.where(nan, 0.0, b).tobytes()


def build_instance(shape, seed=11):
    """Random own arrays and a random (n, N+1, 3) buffer; the local agents are its rows 1 .. B.
    Returns (prm, own, nbr, traj, self_offset)."""
    nx, mo, nb, N, B, ix, iy, iz = shape
    rng = np.random.default_rng(seed)
    n, off = B + 3, 1
    own = dict(qlin_own=rng.standard_normal((B, N + 1, nx)), C_own=rng.standard_normal((B, N, mo, nx)),
               h_own=rng.standard_normal((B, N, mo)))
    traj = rng.standard_normal((n, N + 1, 3))
    nbr = np.zeros((B, nb), np.int32)
    for b in range(B):
        nbr[b] = rng.permutation([j for j in range(n) if j != off + b])[:nb]
    return dict(PRM, ix=ix, iy=iy, iz=iz), own, nbr, traj, off


# (nx, ns, nu, N, B, ix, iy, iz, n_total, self_offset); N = 70: 213 position entries over 64 lanes
PUBLISH_SHAPE = (6, 2, 3, 70, 6, 4, 0, 2, 9, 2)


def nz_of(shape):
    nx, ns, nu, N = shape[:4]
    return (nx + ns) * (N + 1) + 2 * nu * N


def positions(shape, z):
    """new[b, k] = (z[b, k nxe + ix], z[b, k nxe + iy], z[b, k nxe + iz])"""
    nx, ns, nu, N, B, ix, iy, iz = shape[:8]
    xi = z[:, :(nx + ns) * (N + 1)].reshape(B, N + 1, nx + ns)
    return np.stack([xi[:, :, ix], xi[:, :, iy], xi[:, :, iz]], axis=-1)


def publish_instance(shape=PUBLISH_SHAPE, seed=5):
    """Random z; the exchange buffer's local rows are the predicted positions moved by up to 0.005 (even agents: close
    under atol = 0.01) or 0.05 (odd agents: not close).  Planted: agent 0 has a NaN in the last du entry (never
    copied), agent 1 an inf in a slack entry of stage 0, agent 2 a NaN in prev at the last z coordinate (entry 3N + 2,
    past three passes of the lanes), agent 3 negative zeros in z's position entries; agents 4, 5 are plain.
    Returns (prm, z, traj_all, self_offset)."""
    nx, ns, nu, N, B, ix, iy, iz, n, off = shape
    rng = np.random.default_rng(seed)
    nxe = nx + ns
    z = rng.standard_normal((B, nz_of(shape)))
    traj = rng.standard_normal((n, N + 1, 3))
    move = np.where(np.arange(B) % 2 == 0, 0.005, 0.05)[:, None, None]
    z[3, nxe + ix] = z[3, 2 * nxe + iy] = z[3, 3 * nxe + iz] = -0.0
    traj[off:off + B] = positions(shape, z) + move * rng.uniform(-1.0, 1.0, (B, N + 1, 3))
    z[0, -1] = np.nan
    z[1, nx] = np.inf
    traj[off + 2, N, 2] = np.nan
    return dict(PRM, ix=ix, iy=iy, iz=iz), z, traj, off


def population(n, N, seed=11):
    """n agents in a box, drifting: (n, N+1, 3), all distances distinct"""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(-5.0, 5.0, (n, 1, 3))
    v = rng.uniform(-1.0, 1.0, (n, 1, 3))
    return p0 + v * (0.1 * np.arange(N + 1))[None, :, None]


def planted(traj):
    """``traj`` with duplicated points (ties: the index decides; an agent on another's point is a valid neighbour)
    and a NaN coordinate (that agent's scores are NaN, and it is everybody's last choice)."""
    t = traj.copy()
    n = t.shape[0]
    t[n // 2] = t[1]
    t[n - 1] = t[1]
    t[3] = t[2]
    t[5, t.shape[1] - 1, 2] = np.nan
    return t


def brute_select(traj, nb, window, rows):
    """The selection rule written out with loops: (nbr, dist2) of the agents ``rows``."""
    n, k0, k1 = traj.shape[0], window[0], window[1]
    nbr, d2 = np.zeros((len(rows), nb), np.int32), np.zeros((len(rows), nb))
    with np.errstate(invalid="ignore"):
        for r, g in enumerate(rows):
            cand = []
            for j in range(n):
                if j == g:
                    continue
                s = np.inf
                bad = False
                for k in range(k0, k1 + 1):
                    dx, dy, dz = traj[j, k] - traj[g, k]
                    d = dx * dx + dy * dy + dz * dz
                    bad = bad or np.isnan(d)
                    s = min(s, d)
                cand.append((np.inf if bad else s, j))
            cand.sort()
            nbr[r] = [j for _, j in cand[:nb]]
            d2[r] = [s for s, _ in cand[:nb]]
    return nbr, d2
