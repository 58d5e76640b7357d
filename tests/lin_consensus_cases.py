"""What the host and the GPU tests of the consensus step share (tests/test_lin_consensus_host.py, _gpu.py): the
publish kernel's shapes with their planted agents, the threshold pair, and the 9-state stage table of
tests/test_lin_table_gpu.py rebuilt."""
import numpy as np

from cmpc import scenarios as S

# (nx, ns, nu, N, B, ix, iy, n_total, self_offset); the last has 142 position entries: more than the wave has lanes
PUBLISH_SHAPES = [(4, 3, 2, 3, 5, 0, 1, 8, 1), (9, 3, 2, 2, 3, 7, 8, 6, 2), (12, 0, 1, 1, 1, 11, 0, 3, 0),
                  (6, 2, 3, 70, 2, 0, 1, 4, 2)]


def nz_of(shape):
    nx, ns, nu, N = shape[:4]
    return (nx + ns) * (N + 1) + 2 * nu * N


def positions(shape, z):
    """new[b, k] = (z[b, k nxe + ix], z[b, k nxe + iy])"""
    nx, ns, nu, N, B, ix, iy = shape[:7]
    xi = z[:, :(nx + ns) * (N + 1)].reshape(B, N + 1, nx + ns)
    return np.stack([xi[:, :, ix], xi[:, :, iy]], axis=-1)


def publish_instance(shape, seed=5):
    """Random z; the exchange buffer's local rows are the predicted positions moved by up to 0.005 (even agents:
    close under atol = 0.01) or 0.05 (odd agents: not close).  Then the planted agents, by batch size:
      B >= 3: agent 0 has a NaN in the last du entry, agent 1 an inf in a slack entry of stage 0;
      B >= 5: agent 2 has a NaN in prev, agent 3 negative zeros in z's position entries (prev + 0.0 there), agent 4
              is plain (and close);
      B == 2: agent 1 has a NaN in prev at entry 2 (N - 2) + 1, past two passes of the wave's lanes.
    Returns (prm, z, traj_all, self_offset)."""
    nx, ns, nu, N, B, ix, iy, n, off = shape
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, nz_of(shape)))
    traj = rng.standard_normal((n, N + 1, 2))
    move = np.where(np.arange(B) % 2 == 0, 0.005, 0.05)[:, None, None]
    if B >= 5:
        z[3, (nx + ns) + ix] = z[3, 2 * (nx + ns) + iy] = -0.0
    traj[off:off + B] = positions(shape, z) + move * rng.uniform(-1.0, 1.0, (B, N + 1, 2))
    if B >= 3:
        z[0, -1] = np.nan
        z[1, nx] = np.inf
    if B >= 5:
        traj[off + 2, 1, 0] = np.nan
    if B == 2:
        traj[off + 1, N - 2, 1] = np.nan
    return dict(ix=ix, iy=iy, min_dist=0.25, wq=5.0), z, traj, off


ATOL_T = 0.25   # with rtol = 0: |1.0 - 1.25| = 0.25 is close, |1.0 - nextafter(1.25, 2)| is not (both exact in fp64)


def threshold_instance(shape, seed=6):
    """prev = 1.0 everywhere; every agent predicts 1.25 everywhere (close at atol = 0.25, rtol = 0), and an odd agent
    predicts nextafter(1.25, 2) in its last position entry (not close).  Returns (prm, z, traj_all, self_offset)."""
    nx, ns, nu, N, B, ix, iy, n, off = shape
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, nz_of(shape)))
    nxe = nx + ns
    for k in range(N + 1):
        z[:, k * nxe + ix] = z[:, k * nxe + iy] = 1.25
    z[1::2, N * nxe + iy] = np.nextafter(1.25, 2.0)
    traj = rng.standard_normal((n, N + 1, 2))
    traj[off:off + B] = 1.0
    return dict(ix=ix, iy=iy, min_dist=0.25, wq=5.0), z, traj, off


def make_ltv_table(T, n=12, N=10, nb=2, seed=7):
    """The 9-state stage table of tests/test_lin_table_gpu.py (make_ltv_table), rebuilt: 12 agents on the three-lane
    road, x = [v_x, v_y, c2, e_y, c4, c5, c6, X, Y], u = (a_y, a_x); A_tau = I + dt (kinematics + seeded
    perturbation), B_tau likewise; the reference speed rises and the speed bound tightens along the table."""
    rng = np.random.default_rng(seed)
    nx, nu, ns, dt = 9, 2, 3, S.DT
    Ac = np.zeros((nx, nx))
    Ac[7, 0] = Ac[8, 1] = Ac[3, 1] = 1.0
    for c in (2, 4, 5, 6):
        Ac[c, c] = -2.0
    Bc = np.zeros((nx, nu))
    Bc[0, 1] = Bc[1, 0] = 1.0
    Bc[2, 0] = Bc[4, 1] = 0.1
    A = np.eye(nx) + dt * (Ac + 0.02 * rng.standard_normal((n, T, nx, nx)))
    B = dt * (Bc + 0.02 * rng.standard_normal((n, T, nx, nu)))
    i = np.arange(n)
    lane = np.array([S.LANES[k % 3] for k in i])
    x0 = np.zeros((n, nx))
    x0[:, 0] = rng.uniform(1.0, 1.6, n)
    x0[:, 3] = rng.uniform(-0.05, 0.05, n)
    x0[:, 7] = 0.5 * (i // 3) + rng.uniform(-0.05, 0.05, n)
    x0[:, 8] = lane + x0[:, 3]
    x0[:, [2, 4, 5, 6]] = 0.01 * rng.standard_normal((n, 4))
    k = np.arange(N + 1)[None, :]
    traj = np.stack([x0[:, 7:8] + k * dt * x0[:, 0:1], x0[:, 8:9] + 0 * k], axis=-1)
    Q = np.diag([10.0, 1.0, 0.1, 25.0, 0.1, 0.1, 0.1, 0.0, 0.0])
    shared = dict(nx=nx, nu=nu, N=N, ns=ns, mc=4 + nb, Q=Q, R=np.zeros((nu, nu)), dR=50.0 * np.eye(nu),
                  Qs=np.full(3, 1e7), u_ub=np.array([5.0, 5.0]), u_lb=np.array([-5.0, -10.0]),
                  row_slack=np.array([-1, 0, 1, 1] + [2] * nb, np.int32),
                  row_sign=np.array([1, 1, 1, 1] + [-1] * nb, np.int32))
    tau = np.arange(T)
    C = np.zeros((n, T, 4, nx))
    C[:, :, 0, 0], C[:, :, 1, 0], C[:, :, 2, 3], C[:, :, 3, 3] = -1.0, 1.0, 1.0, -1.0
    h = np.broadcast_to(np.array([-0.0, 5.5, 0.75, 0.75]), (n, T, 4)).copy()
    h[:, :, 1] = 5.5 - 0.02 * tau
    qlin = np.zeros((n, T, nx))
    qlin[:, :, 0] = -10.0 * (3.0 + 0.05 * tau)
    return dict(shared=shared, prm=dict(ix=7, iy=8, min_dist=0.25, wq=5.0), table=dict(A=A, B=B, qlin=qlin, C=C, h=h),
                T=T, x0=x0, u_prev=np.zeros((n, nu)), nbr=S.nearest_neighbours(x0[:, 7:9], nb), traj=traj)
