"""Synthetic agent populations for BASELINE.json configs 1-5.

Double integrator x = [p (dim) | v (dim)], u = a (dim), dt = 0.025 (the
reference's sample time, planner/scripts/config_files/config_LPV.py:22).  Cost
and limits mirror the reference's roles (config_LPV.py:6-11, config/base_class.py:
30-41): 10 on (v_x - v_ref) with v_ref = 3.0, 25 on (p_y - lane), R = 0,
dR = 50 I, Qs = 1e7, accel 5 / decel 10 on a_x and |a| <= 5 on the others,
soft speed cap 5.5, soft lane half-width 0.75 (Highway halfWidth,
mapManager/track_initialization.py:112), soft collision half-planes d = 0.25,
coverage weight wq = 5.

Agents sit on a straight 3-lane road: p_x = 0.5 floor(i/3) + U(-.05,.05),
p_y = {-0.5, 0, 0.5}[i%3] + U(-.05,.05), v_x ~ U(1.0, 1.6), v_y = 0, drawn from
numpy.random.default_rng(20240101) in that order.  Neighbours: the nb nearest
agents by initial position (a fixed graph unless the rounds re-select it: `select_neighbours`,
`rounds.DIRounds(reselect=r)`).  Previous predictions: constant-velocity
rollout, as initialise_agents does (utilities/misc.py:155-210).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

DT = 0.025
SEED = 20240101
LANES = (-0.5, 0.0, 0.5)


def di_params(dim=2):
    return dict(dim=dim, v_ref=3.0, q_v=10.0, q_lane=25.0, hw=0.75, min_vel=0.0, max_vel=5.5,
                min_dist=0.25, wq=5.0)


def di_shared(dim, N, nb):
    nx, nu = 2 * dim, dim
    prm = di_params(dim)
    Q = np.zeros((nx, nx))
    Q[1, 1] = prm["q_lane"]
    Q[dim, dim] = prm["q_v"]
    ub = np.full(nu, 5.0)
    lb = np.full(nu, -5.0)
    lb[0] = -10.0
    return dict(nx=nx, nu=nu, N=N, ns=3, mc=4 + nb, Q=Q, R=np.zeros((nu, nu)), dR=50.0 * np.eye(nu),
                Qs=np.full(3, 1e7), u_ub=ub, u_lb=lb,
                row_slack=np.array([-1, 0, 1, 1] + [2] * nb, np.int32),
                row_sign=np.array([1, 1, 1, 1] + [-1] * nb, np.int32))


def di_dynamics(dim, dt=DT):
    I = np.eye(dim)
    A = np.block([[I, dt * I], [np.zeros((dim, dim)), I]])
    B = np.vstack([0.5 * dt * dt * I, dt * I])
    return A, B


@dataclass
class DIScenario:
    dim: int
    N: int
    nb: int
    n_agents: int
    params: dict
    shared: dict
    A: np.ndarray       # (n, N, nx, nx)
    B: np.ndarray       # (n, N, nx, nu)
    x0: np.ndarray      # (n, nx)
    u_prev: np.ndarray  # (n, nu)
    lane: np.ndarray    # (n,)
    nbr: np.ndarray     # (n, nb) int32 global indices
    traj: np.ndarray    # (n, N+1, 2) previous predicted positions
    extra: dict = field(default_factory=dict)

    def shard(self, rank, world):
        """Contiguous block of agents owned by `rank` (agents are ordered along the road,
        so most neighbours live on the same GPU)."""
        per = self.n_agents // world
        return slice(rank * per, (rank + 1) * per)


def nearest_neighbours(pos, nb):
    from scipy.spatial import cKDTree

    n = pos.shape[0]
    if nb == 0:
        return np.zeros((n, 0), np.int32)
    if nb >= n:
        raise ValueError("need more agents than neighbours")
    _, idx = cKDTree(pos).query(pos, k=nb + 1)
    out = np.zeros((n, nb), np.int32)
    for i in range(n):
        row = [j for j in idx[i] if j != i][:nb]
        out[i] = row
    return out


def select_neighbours(traj, nb, window=(0, 0), rows=None, return_dist2=False):
    """Host statement of the device neighbour selection (cmpc_nbr_select_dev, include/cmpc.h): for every
    agent g in ``rows`` (default: all) the ``nb`` nearest other agents of ``traj`` (n, N+1, 2).

    score(g, j) = min over the stages k0..k1 of ``window`` of dx*dx + dy*dy (numpy's min: a NaN at any
    stage of the window makes the score NaN); a NaN score counts as +inf; candidates are ordered by
    (score, j) ascending and j = g is left out by index, never by distance.  Returns (len(rows), nb)
    int32 global indices, nearest first (and their scores with ``return_dist2``).  Window (0, 0) is
    "nearest now" — on distinct distances what ``nearest_neighbours`` gives for the stage-0 positions;
    (0, N) is the closest predicted approach.  The reference's ns[i] (LPV_HP_N_main.py:82-85) is in
    index order: nearest first only reorders an agent's collision rows and the columns of ``planes``.
    A buffer (n, N+1, 3) is scored by dx*dx + dy*dy + dz*dz, summed left to right (cmpc_nbr_select3_dev)."""
    traj = np.asarray(traj, np.float64)
    n, (k0, k1) = traj.shape[0], window
    if not (0 <= k0 <= k1 < traj.shape[1]) or not (0 <= nb < n):
        raise ValueError("need 0 <= k0 <= k1 <= N and 0 <= nb < n")
    rows = np.arange(n) if rows is None else np.arange(n)[rows]
    w = traj[:, k0:k1 + 1]
    score = np.empty((len(rows), n))
    step = max(1, (1 << 22) // (n * w.shape[1]))           # rows per block: bounds the (block, n, stages) arrays
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, len(rows), step):
            r = rows[i:i + step]
            dx = w[None, :, :, 0] - w[r, None, :, 0]
            dy = w[None, :, :, 1] - w[r, None, :, 1]
            d2 = dx * dx + dy * dy
            if traj.shape[2] == 3:
                dz = w[None, :, :, 2] - w[r, None, :, 2]
                d2 = d2 + dz * dz
            score[i:i + step] = d2.min(axis=2)
    score[np.isnan(score)] = np.inf
    j = np.broadcast_to(np.arange(n), score.shape)
    order = np.lexsort((j, score), axis=1)                 # by score, then by index
    order = order[order != rows[:, None]].reshape(len(rows), n - 1)[:, :nb]
    idx = order.astype(np.int32)
    return (idx, np.take_along_axis(score, order, axis=1)) if return_dist2 else idx


def order_by_iters(iters):
    """Host statement of the device launch order (cmpc_order_by_iters_dev, include/cmpc.h): the agents by
    descending key = min(max(iters, 0), 65535), equal keys in index order — the permutation
    ``cmpc_opts.order`` takes (last round's longest solves first).  For keys in range it is
    ``torch.argsort(iters, descending=True, stable=True)``.  Returns (len(iters),) int32."""
    return np.argsort(-np.clip(np.asarray(iters, np.int64), 0, 65535), kind="stable").astype(np.int32)


def log_row(z, nx, nu, ns, N, look_col):
    """Host statement of a round's log rows (cmpc_round_log_dev, include/cmpc.h) from the round's ``z``
    (batch, nz) in the reference layout, nz = (nx+ns)(N+1) + 2 nu N: what the reference appends per control step
    to states.dat / u.dat / plan_dist.dat (config/base_class.py:64-99).  Returns (state, u, look_ahead):
    state (batch, nx) = xPred[0], u (batch, nu) = uPred[0], look_ahead (batch,) =
    xPred[-1, look_col] - xPred[0, look_col].  Copies, bit for bit; the look-ahead is one subtraction."""
    z = np.asarray(z, np.float64)
    nxe = nx + ns
    if z.ndim != 2 or z.shape[1] != nxe * (N + 1) + 2 * nu * N or not (0 <= look_col < nx):
        raise ValueError("z: (batch, (nx+ns)(N+1) + 2 nu N), 0 <= look_col < nx")
    u0 = nxe * (N + 1)
    with np.errstate(invalid="ignore"):
        look = z[:, nxe * N + look_col] - z[:, look_col]
    return z[:, :nx].copy(), z[:, u0:u0 + nu].copy(), look


def lin_rows(prm, own, nbr, traj, self_offset=0):
    """Host statement of the linear-model family's builder (cmpc_lin_build_dev, include/cmpc.h), every expression
    in the header's order, each numpy operation rounded once (no fma).  ``prm``: dict(ix, iy, min_dist, wq);
    ``own``: dict(qlin_own (B, N+1, nx), C_own (B, N, mo, nx), h_own (B, N, mo)), C_own / h_own may be None when
    the agents have no own rows; ``nbr`` (B, nb) global indices into ``traj`` (n_total, N+1, 2); the local agents
    are rows self_offset .. self_offset + B of ``traj``.  Returns (qlin (B, N+1, nx), C (B, N, mo+nb, nx),
    h (B, N, mo+nb)).  A neighbour on the agent's own point gives NaN rows and cost at that stage.
    A ``prm`` with the key ``iz`` selects the 3-D rule (cmpc_lin3_build_dev): ``traj`` is (n_total, N+1, 3), the
    third coordinate joins every sum (left to right) and column iz gets the normal's third component."""
    if "iz" in prm:
        return _lin3_rows(prm, own, nbr, traj, self_offset)
    ix, iy, d, wq = int(prm["ix"]), int(prm["iy"]), float(prm["min_dist"]), float(prm["wq"])
    q_own = np.asarray(own["qlin_own"], np.float64)
    B, N, nx = q_own.shape[0], q_own.shape[1] - 1, q_own.shape[2]
    C_own = np.zeros((B, N, 0, nx)) if own.get("C_own") is None else np.asarray(own["C_own"], np.float64)
    h_own = np.zeros((B, N, 0)) if own.get("h_own") is None else np.asarray(own["h_own"], np.float64)
    mo = C_own.shape[2]
    nbr = np.asarray(nbr, np.int64).reshape(B, -1)
    nb = nbr.shape[1]
    traj = np.asarray(traj, np.float64)
    if not (0 <= ix < nx and 0 <= iy < nx and ix != iy) or C_own.shape != (B, N, mo, nx) or h_own.shape != (B, N, mo) \
            or traj.shape[1:] != (N + 1, 2):
        raise ValueError("lin_rows: ix != iy in [0, nx), C_own (B, N, mo, nx), h_own (B, N, mo), traj (n, N+1, 2)")
    C = np.zeros((B, N, mo + nb, nx))
    h = np.zeros((B, N, mo + nb))
    C[:, :, :mo] = C_own
    h[:, :, :mo] = h_own
    me = traj[self_offset:self_offset + B]
    px, py = np.zeros((B, N)), np.zeros((B, N))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(nb):
            nt = traj[nbr[:, i]]
            ex, ey, nx_, ny_ = me[:, :-1, 0], me[:, :-1, 1], nt[:, :-1, 0], nt[:, :-1, 1]   # planes: row k-1
            dx, dy = nx_ - ex, ny_ - ey
            nrm = np.sqrt(dx * dx + dy * dy)
            ax, ay = dx / nrm, dy / nrm
            bb = -0.5 * (ax * (ex + nx_) + ay * (ey + ny_))
            qx, qy = me[:, 1:, 0] - nt[:, 1:, 0], me[:, 1:, 1] - nt[:, 1:, 1]               # weights: row k
            wgt = (2.0 * d - np.sqrt(qx * qx + qy * qy)) / nb
            C[:, :, mo + i, ix] = ax
            C[:, :, mo + i, iy] = ay
            h[:, :, mo + i] = -d / 2 - bb
            px = px + wq * wgt * ax
            py = py + wq * wgt * ay
        qlin = q_own.copy()
        qlin[:, 1:, ix] = q_own[:, 1:, ix] + px
        qlin[:, 1:, iy] = q_own[:, 1:, iy] + py
    return qlin, C, h


def _pos3(prm, nx):
    """The three position columns of a 3-D ``prm``, checked: pairwise different, each in [0, nx)."""
    cols = tuple(int(prm[k]) for k in ("ix", "iy", "iz"))
    if len(set(cols)) != 3 or not all(0 <= c < nx for c in cols):
        raise ValueError("position columns ix, iy, iz: pairwise different, each in [0, nx)")
    return cols


def _lin3_rows(prm, own, nbr, traj, self_offset=0):
    """``lin_rows`` for a ``prm`` with ``iz`` (cmpc_lin3_build_dev, include/cmpc.h): the same statement with three
    coordinates, every sum left to right."""
    d, wq = float(prm["min_dist"]), float(prm["wq"])
    q_own = np.asarray(own["qlin_own"], np.float64)
    B, N, nx = q_own.shape[0], q_own.shape[1] - 1, q_own.shape[2]
    C_own = np.zeros((B, N, 0, nx)) if own.get("C_own") is None else np.asarray(own["C_own"], np.float64)
    h_own = np.zeros((B, N, 0)) if own.get("h_own") is None else np.asarray(own["h_own"], np.float64)
    mo = C_own.shape[2]
    nbr = np.asarray(nbr, np.int64).reshape(B, -1)
    nb = nbr.shape[1]
    traj = np.asarray(traj, np.float64)
    ix, iy, iz = _pos3(prm, nx)
    if C_own.shape != (B, N, mo, nx) or h_own.shape != (B, N, mo) or traj.ndim != 3 or traj.shape[1:] != (N + 1, 3):
        raise ValueError("lin_rows (3-D): C_own (B, N, mo, nx), h_own (B, N, mo), traj (n, N+1, 3)")
    C = np.zeros((B, N, mo + nb, nx))
    h = np.zeros((B, N, mo + nb))
    C[:, :, :mo] = C_own
    h[:, :, :mo] = h_own
    me = traj[self_offset:self_offset + B]
    px, py, pz = np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(nb):
            nt = traj[nbr[:, i]]
            ex, ey, ez = (me[:, :-1, c] for c in range(3))                                  # planes: row k-1
            nx_, ny_, nz_ = (nt[:, :-1, c] for c in range(3))
            dx, dy, dz = nx_ - ex, ny_ - ey, nz_ - ez
            nrm = np.sqrt(dx * dx + dy * dy + dz * dz)
            ax, ay, az = dx / nrm, dy / nrm, dz / nrm
            bb = -0.5 * (ax * (ex + nx_) + ay * (ey + ny_) + az * (ez + nz_))
            qx, qy, qz = (me[:, 1:, c] - nt[:, 1:, c] for c in range(3))                    # weights: row k
            wgt = (2.0 * d - np.sqrt(qx * qx + qy * qy + qz * qz)) / nb
            C[:, :, mo + i, ix] = ax
            C[:, :, mo + i, iy] = ay
            C[:, :, mo + i, iz] = az
            h[:, :, mo + i] = -d / 2 - bb
            px = px + wq * wgt * ax
            py = py + wq * wgt * ay
            pz = pz + wq * wgt * az
        qlin = q_own.copy()
        qlin[:, 1:, ix] = q_own[:, 1:, ix] + px
        qlin[:, 1:, iy] = q_own[:, 1:, iy] + py
        qlin[:, 1:, iz] = q_own[:, 1:, iz] + pz
    return qlin, C, h


def _positions(prm, xi):
    """The predicted positions (B, N+1, 2 | 3) out of the stage states ``xi`` (B, N+1, nxe): columns ix, iy, and
    iz when ``prm`` has it."""
    cols = [int(prm["ix"]), int(prm["iy"])] + ([int(prm["iz"])] if "iz" in prm else [])
    return np.stack([xi[:, :, c] for c in cols], axis=-1)


def lin_advance(prm, z, nx, nu, ns, N, x0, u_prev, traj_local):
    """Host statement of the family's advance (cmpc_lin_advance_dev): from ``z`` (B, nz) in the reference layout,
    nxe = nx + ns: x0 <- z[nxe : nxe+nx], u_prev <- z[nxe(N+1) : +nu], traj_local[k] <- (z[k nxe + ix],
    z[k nxe + iy]).  An agent whose z holds any non-finite value keeps all three.  Returns new (x0, u_prev,
    traj_local); the arguments are left alone.  With ``iz`` in ``prm`` (cmpc_lin3_advance_dev) traj_local is
    (B, N+1, 3) and traj_local[k] <- (z[k nxe + ix], z[k nxe + iy], z[k nxe + iz])."""
    z = np.asarray(z, np.float64)
    ix, iy, nxe = int(prm["ix"]), int(prm["iy"]), nx + ns
    if z.ndim != 2 or z.shape[1] != nxe * (N + 1) + 2 * nu * N:
        raise ValueError("z: (batch, (nx+ns)(N+1) + 2 nu N)")
    x0, u_prev, traj_local = (np.array(a, np.float64) for a in (x0, u_prev, traj_local))
    if "iz" in prm and (_pos3(prm, nx) and traj_local.shape != (z.shape[0], N + 1, 3)):
        raise ValueError("lin_advance (3-D): traj_local (B, N+1, 3)")
    ok = np.isfinite(z).all(axis=1)
    xi = z[:, :nxe * (N + 1)].reshape(-1, N + 1, nxe)
    x0[ok] = xi[ok, 1, :nx]
    u_prev[ok] = z[ok, nxe * (N + 1):nxe * (N + 1) + nu]
    if "iz" in prm:
        traj_local[ok] = _positions(prm, xi[ok])
    else:
        traj_local[ok] = np.stack([xi[ok, :, ix], xi[ok, :, iy]], axis=-1)
    return x0, u_prev, traj_local


def lin_publish(prm, z, nx, nu, ns, N, traj_all, atol=0.01, rtol=1e-5, self_offset=0):
    """Host statement of an inner round's publication (cmpc_lin_publish_dev, include/cmpc.h), every expression
    rounded as written.  ``z`` (B, nz) in the reference layout, ``traj_all`` (n_total, N+1, 2); the local agents are
    rows self_offset .. self_offset + B of it (``prev``).  With new[k] = (z[k nxe + ix], z[k nxe + iy]): an agent
    whose z holds any non-finite value publishes ``prev`` again, with close = 0 and delta = NaN; every other agent
    publishes ``new``, close = all(|prev - new| <= atol + rtol |new|) (numpy's allclose: a NaN is never close) and
    delta = max |prev - new| (numpy's max: NaN when any term is).  Returns (traj_local (B, N+1, 2), close (B,) int32,
    delta (B,), not_close = the number of agents with close == 0); the arguments are left alone.  With ``iz`` in
    ``prm`` (cmpc_lin3_publish_dev) the buffers are x 3 and new[k] has z[k nxe + iz] as its third entry."""
    z, traj_all = np.asarray(z, np.float64), np.asarray(traj_all, np.float64)
    ix, iy, nxe, off = int(prm["ix"]), int(prm["iy"]), nx + ns, int(self_offset)
    pd = 3 if "iz" in prm else 2
    if pd == 3:
        _pos3(prm, nx)
    if z.ndim != 2 or z.shape[1] != nxe * (N + 1) + 2 * nu * N or traj_all.ndim != 3 or \
            traj_all.shape[1:] != (N + 1, pd) or not (0 <= off and off + z.shape[0] <= traj_all.shape[0]) or \
            not (0 <= ix < nx and 0 <= iy < nx and ix != iy) or not (atol >= 0 and rtol >= 0):
        raise ValueError(f"lin_publish: z (B, (nx+ns)(N+1) + 2 nu N), traj_all (n_total >= self_offset + B, N+1, {pd}), "
                         "ix != iy in [0, nx), atol, rtol >= 0")
    B = z.shape[0]
    prev = traj_all[off:off + B]
    ok = np.isfinite(z).all(axis=1)
    xi = z[:, :nxe * (N + 1)].reshape(B, N + 1, nxe)
    new = _positions(prm, xi)
    traj_local = np.where(ok[:, None, None], new, prev)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(prev - traj_local).reshape(B, -1)
        lim = (atol + rtol * np.abs(traj_local)).reshape(B, -1)
        close = ((d <= lim).all(axis=1) & ok).astype(np.int32)
        delta = np.where(ok, d.max(axis=1), np.nan)
    return traj_local, close, delta, int((close == 0).sum())


def consensus_stop(not_close, min_rounds=3, need=2, max_rounds=12):
    """The stopping rule of a consensus step (cmpc_lin_rounds_step_consensus, include/cmpc.h) as a pure function of
    the node-wide ``not_close`` counts of the inner rounds 1..j run so far (j = len(not_close) >= 1).  Round 1 is
    not compared; for rounds >= 2 ``streak`` counts the consecutive rounds, ending at the current one, whose count
    was 0; ``agreed`` turns true the first time streak >= need and stays true; the step stops after round j when
    j >= max_rounds, or when agreed and j >= min_rounds.  Returns (stop, agreed).  ``ocd.OCDLoopState`` with
    min_rounds = min_it_OCD + 1, need = it_conv + 1, max_rounds = max_it_OCD + 2 (the defaults are the
    reference's)."""
    j = len(not_close)
    if j < 1 or min_rounds < 1 or need < 1 or max_rounds < min_rounds:
        raise ValueError("consensus_stop: at least one round, 1 <= min_rounds <= max_rounds, need >= 1")
    streak, agreed = 0, False
    for c in list(not_close)[1:]:
        streak = streak + 1 if int(c) == 0 else 0
        agreed = agreed or streak >= need
    return bool(j >= max_rounds or (agreed and j >= min_rounds)), bool(agreed)


LPV_PUBLISH = dict(prm=dict(ix=7, iy=8), nx=9, nu=2, ns=3)   # the LPV agents' z layout in lin_publish's terms


def lpv_publish(z, N, traj_all, status=None, atol=0.01, rtol=1e-5, self_offset=0):
    """Host statement of an inner round's publication on the LPV handles (cmpc_lpv_publish_dev, include/cmpc.h):
    ``lin_publish`` on the LPV layout (positions in state columns 7, 8 of 9 states + 3 slacks per stage, 2 inputs:
    nz = 12(N+1) + 4N), plus the reference's feasibility rule on ``status`` (B,): an agent whose status is not in
    {1, 2, -2} is infeasible (LPV_Planner.py:243-249, what cmpc_lpv_advance_dev counts).  Returns (traj_local
    (B, N+1, 2), close (B,) int32, delta (B,), not_close, infeasible); infeasible is 0 when ``status`` is None."""
    c = LPV_PUBLISH
    traj_local, close, delta, not_close = lin_publish(c["prm"], z, c["nx"], c["nu"], c["ns"], N, traj_all, atol=atol,
                                                      rtol=rtol, self_offset=self_offset)
    infeasible = 0
    if status is not None:
        status = np.asarray(status)
        if status.shape != (close.shape[0],):
            raise ValueError("lpv_publish: status (B,)")
        infeasible = int((~np.isin(status, (1, 2, -2))).sum())
    return traj_local, close, delta, not_close, infeasible


def lin_of_di(scen, rows=None):
    """A ``DIScenario`` in the linear-model family: the arguments of ``lin_rows`` (and of cmpc_lin_build_dev) that
    give the double-integrator builder's qlin, C, h bit for bit.  Position columns ix, iy = 0, 1; mo = 4 own rows
    per stage, [-v_x <= -min_vel; v_x <= max_vel; p_y <= hw + lane; -p_y <= hw - lane]; own cost -v_ref q_v on v_x
    and -lane q_lane on p_y, exact 0.0 elsewhere; min_dist and wq from the scenario's parameters.  ``rows``: the
    local agents (a slice, default all).  Returns dict(prm, own, nbr, traj, self_offset)."""
    p, dim, N = scen.params, scen.dim, scen.N
    sl = slice(0, scen.n_agents) if rows is None else rows
    lane = np.asarray(scen.lane, np.float64)[sl]
    B, nx = lane.shape[0], 2 * dim
    C_own = np.zeros((B, N, 4, nx))
    C_own[:, :, 0, dim] = -1.0
    C_own[:, :, 1, dim] = 1.0
    C_own[:, :, 2, 1] = 1.0
    C_own[:, :, 3, 1] = -1.0
    h_own = np.empty((B, N, 4))
    h_own[:, :, 0] = -p["min_vel"]
    h_own[:, :, 1] = p["max_vel"]
    h_own[:, :, 2] = (p["hw"] + lane)[:, None]
    h_own[:, :, 3] = (p["hw"] - lane)[:, None]
    qlin_own = np.zeros((B, N + 1, nx))
    qlin_own[:, :, dim] = -p["v_ref"] * p["q_v"]
    qlin_own[:, :, 1] = (-lane * p["q_lane"])[:, None]
    return dict(prm=dict(ix=0, iy=1, min_dist=p["min_dist"], wq=p["wq"]),
                own=dict(qlin_own=qlin_own, C_own=C_own, h_own=h_own), nbr=np.asarray(scen.nbr)[sl], traj=scen.traj,
                self_offset=sl.start or 0)


def rollout3(x0, N, dim=3, dt=DT):
    """The constant-velocity rollout of 3-D double-integrator states ``x0`` (n, 2 dim), dim >= 3: (n, N+1, 3)
    positions x0[:, c] + k dt x0[:, dim + c], c = 0, 1, 2 (``make_di``'s rollout with the third column)."""
    x0 = np.asarray(x0, np.float64)
    k = np.arange(N + 1)[None, :]
    return np.stack([x0[:, c:c + 1] + k * dt * x0[:, dim + c:dim + c + 1] for c in range(3)], axis=-1)


def lin3_of_di(scen, alt, rows=None):
    """A 3-D ``DIScenario`` (``dim == 3``) in the linear-model family with 3-D positions (cmpc_lin3_*):
    ``lin_of_di``'s dict with prm["iz"] = 2, ``x0`` = the scenario's states with column 2 (the altitude) set to
    ``alt`` (a scalar or (n,)), and ``traj`` = their constant-velocity rollout with three columns (n, N+1, 3).
    With one altitude for everybody the rows and the cost are ``lin_of_di``'s, bit for bit."""
    if scen.dim != 3:
        raise ValueError("lin3_of_di: a scenario with dim == 3")
    lin = lin_of_di(scen, rows)
    x0 = np.array(scen.x0, np.float64)
    x0[:, 2] = alt
    lin["prm"]["iz"] = 2
    lin.update(x0=x0, traj=rollout3(x0, scen.N, scen.dim))
    return lin


def make_stacked(n_agents, N, nb=2, gap=0.6):
    """A population the planar rule cannot separate: ``make_di(n_agents, N, nb, 3)`` with every odd agent over the
    even agent before it (its ground position, velocity and lane) at altitude ``gap``, the even ones at 0 — pairs
    on one ground point, ``gap`` apart.  ``traj`` is the 3-column constant-velocity rollout and ``nbr`` the 3-D
    selection on window (0, 0).  Returns dict(shared, prm, own, A, B, x0, u_prev, nbr, traj) in the 3-D family
    (prm has ``iz``): the arguments of ``rounds.LinRoundsHandle``."""
    if n_agents < 2 or n_agents % 2:
        raise ValueError("make_stacked: an even number of agents")
    sc = make_di(n_agents, N, nb, 3)
    i = np.arange(n_agents)
    below = i - i % 2
    sc.x0 = sc.x0[below].copy()
    sc.lane = sc.lane[below].copy()
    lin = lin3_of_di(sc, gap * (i % 2))
    return dict(shared=sc.shared, prm=lin["prm"], own=lin["own"], A=sc.A, B=sc.B, x0=lin["x0"], u_prev=sc.u_prev,
                nbr=select_neighbours(lin["traj"], nb), traj=lin["traj"])


TABLE_HOLD, TABLE_PERIODIC = 0, 1   # CMPC_TABLE_HOLD, CMPC_TABLE_PERIODIC


def lin_table_rows(T, t, n, mode=TABLE_HOLD):
    """The stage-table rule of include/cmpc.h: the table rows of the ``n`` absolute stages t, t+1, .., t+n-1 of a
    table of ``T`` rows — tau mod T (``TABLE_PERIODIC``) or min(tau, T-1) (``TABLE_HOLD``: past its end the table
    holds its last stage).  Returns an (n,) int64 index vector."""
    T, t, n, mode = int(T), int(t), int(n), int(mode)
    if T < 1 or t < 0 or n < 0 or mode not in (TABLE_HOLD, TABLE_PERIODIC):
        raise ValueError("lin_table_rows: T >= 1, t >= 0, n >= 0, mode TABLE_HOLD or TABLE_PERIODIC")
    tau = t + np.arange(n, dtype=np.int64)
    return tau % T if mode == TABLE_PERIODIC else np.minimum(tau, T - 1)


def lin_table_rows_of(table):
    """The number of rows T of a stage table, after checking that its arrays agree: ``table`` is dict(A (B, T, nx,
    nx), B (B, T, nx, nu), qlin (B, T, nx), C (B, T, mo, nx), h (B, T, mo)), C / h None (or absent) when the
    agents have no own rows."""
    A, Bm, q = (np.asarray(table[k]) for k in ("A", "B", "qlin"))
    C, h = table.get("C"), table.get("h")
    if A.ndim != 4 or Bm.ndim != 4 or q.ndim != 3 or (C is None) != (h is None):
        raise ValueError("table: A (B, T, nx, nx), B (B, T, nx, nu), qlin (B, T, nx), C (B, T, mo, nx), h (B, T, mo)")
    n, T, nx = q.shape
    ok = T >= 1 and A.shape == (n, T, nx, nx) and Bm.shape[:3] == (n, T, nx)
    if C is not None:
        C, h = np.asarray(C), np.asarray(h)
        ok = ok and C.ndim == 4 and C.shape[:2] == (n, T) and C.shape[3] == nx and h.shape == C.shape[:3]
    if not ok:
        raise ValueError("table: A (B, T, nx, nx), B (B, T, nx, nu), qlin (B, T, nx), C (B, T, mo, nx), h (B, T, mo)")
    return T


def lin_window(table, t, N, mode=TABLE_HOLD):
    """Host statement of the window of a stage table at time ``t`` (cmpc_lin_table_build_dev, include/cmpc.h):
    A_win[b,k] = A[b,row(t+k)], B likewise (k = 0..N-1), qlin_own[b,k] = qlin[b,row(t+k)] (k = 0..N),
    C_own[b,k-1] = C[b,row(t+k)], h_own likewise (k = 1..N); copies, bit for bit.  Returns (A (B, N, nx, nx),
    B (B, N, nx, nu), own) with ``own`` in ``lin_rows``' form."""
    T, N = lin_table_rows_of(table), int(N)
    if N < 1:
        raise ValueError("lin_window: N >= 1")
    r = lin_table_rows(T, t, N + 1, mode)
    C, h = table.get("C"), table.get("h")
    own = dict(qlin_own=np.asarray(table["qlin"], np.float64)[:, r].copy(),
               C_own=None if C is None else np.asarray(C, np.float64)[:, r[1:]].copy(),
               h_own=None if h is None else np.asarray(h, np.float64)[:, r[1:]].copy())
    return np.asarray(table["A"], np.float64)[:, r[:-1]].copy(), np.asarray(table["B"], np.float64)[:, r[:-1]].copy(), own


def lin_table_of_di(scen, T=1, rows=None):
    """A ``DIScenario`` as a stage table: ``lin_of_di``'s arrays are constant over stages, so one row under
    ``TABLE_HOLD`` is the double integrator again (``lin_window`` at any t gives ``lin_of_di``'s arrays and the
    scenario's A, B, bit for bit); ``T`` > 1 repeats that row.  Returns ``lin_of_di``'s dict with ``table`` =
    dict(A, B, qlin, C, h) and ``mode`` in place of ``own``."""
    lin = lin_of_di(scen, rows)
    sl = slice(0, scen.n_agents) if rows is None else rows
    if int(T) < 1 or any((np.asarray(a)[sl] != np.asarray(a)[sl][:, :1]).any() for a in (scen.A, scen.B)):
        raise ValueError("lin_table_of_di: T >= 1, and a scenario whose A, B are the same at every stage")
    own = lin.pop("own")
    rep = lambda a: np.repeat(np.asarray(a, np.float64)[:, :1], int(T), axis=1)   # noqa: E731
    lin.update(table=dict(A=rep(scen.A[sl]), B=rep(scen.B[sl]), qlin=rep(own["qlin_own"]), C=rep(own["C_own"]),
                          h=rep(own["h_own"])), mode=TABLE_HOLD)
    return lin


def make_di(n_agents, N, nb=2, dim=2, seed=SEED):
    rng = np.random.default_rng(seed)
    nx, nu = 2 * dim, dim
    i = np.arange(n_agents)
    ds = rng.uniform(-0.05, 0.05, n_agents)
    dl = rng.uniform(-0.05, 0.05, n_agents)
    vx = rng.uniform(1.0, 1.6, n_agents)
    lane = np.array([LANES[k % 3] for k in i])
    x0 = np.zeros((n_agents, nx))
    x0[:, 0] = 0.5 * (i // 3) + ds
    x0[:, 1] = lane + dl
    x0[:, dim] = vx
    Ad, Bd = di_dynamics(dim)
    A = np.broadcast_to(Ad, (n_agents, N, nx, nx)).copy()
    B = np.broadcast_to(Bd, (n_agents, N, nx, nu)).copy()
    k = np.arange(N + 1)[None, :]
    traj = np.stack([x0[:, 0:1] + k * DT * x0[:, dim:dim + 1],
                     x0[:, 1:2] + k * DT * x0[:, dim + 1:dim + 2]], axis=-1)
    nbr = nearest_neighbours(x0[:, :2], nb)
    return DIScenario(dim, N, nb, n_agents, di_params(dim), di_shared(dim, N, nb), A, B, x0,
                      np.zeros((n_agents, nu)), lane, nbr, traj)


def di_alg_bytes(nx, nu, N, nb, word=8):
    """Algorithmic HBM bytes per agent-QP (SURVEY.md §8d formula)."""
    return word * (N * (nx * nx + nx * nu) + (N + 1) * nx + N * nu + nx + nu + (N + 1) + 2 * nb * (N + 1)
                   + N * nu + (N + 1) * nx + 3 * N + 2)


def riccati_flops(nx, nu, N, iters):
    """Algorithmic flops per agent-QP of the stage-wise Riccati method (mpc_riccati.hip): per IPM
    iteration one factorisation, N x (P[A|B] + [A|B]'T + Hvy'K: 2 na nc nx + nc^2 nx + na^2 nu,
    na = nc = nx + nu), and two Newton solves of 2 sweeps each (4 N (2 nx na)), plus the two
    residual adjoints (2 N 2 nx (nx + nu)).  Used for cfg5's roofline instead of the condensed
    count, which would credit the Riccati kernel with work it does not do."""
    na = nx + nu
    per_it = N * (2 * na * na * nx + na * na * nx + na * na * nu) + 4 * N * 2 * nx * na + 2 * N * 2 * nx * na
    return iters * per_it


def alg_flops(nx, nu, N, ncons, iters):
    """Algorithmic flops per agent-QP: condensing + iters x (G'WG + Cholesky + ...)."""
    n = N * nu
    condense = 2 * N * N * nx * nx * nu + N * nx * n * n + 4 * N * nx * n
    per_it = N * nx * n * n + n ** 3 / 3 + 4 * n * n + 2 * ncons * n
    return condense + iters * per_it
