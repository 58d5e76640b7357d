"""What the host and the GPU tests of the LPV handles' consensus step share (tests/test_lpv_consensus_host.py,
_gpu.py) with tools/lpv_consensus_lab.py: the publish kernel's shapes with their planted agents, the threshold
instances, the captured reference cases, and the CPU loop of a consensus step (numpy builder oracle/lpv_ref.py, C
solver oracle/cmpc_oracle.c under the rescue policy) under both linearisation rules."""
import os

import numpy as np

from cmpc import scenarios as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (N, B, n_total, self_offset): one agent; an offset shard; 2(N+1) = 64 entries, exactly one pass of the wave; 66
# entries, a second pass
PUBLISH_SHAPES = [(1, 1, 1, 0), (10, 2, 5, 3), (31, 3, 4, 1), (32, 5, 8, 2)]
PLANTS = ("plain", "z_last_nan", "slack_inf", "u_neg_inf", "prev_nan", "prev_inf")
STATUSES = (1, 2, -2, -3, -10, 0, 7)          # the first three are feasible (LPV_Planner.py:243-249)
DEFAULTS = dict(min_rounds=3, need=2, max_rounds=12, atol=0.01, rtol=1e-5)


def nz_of(N):
    return 12 * (N + 1) + 4 * N


def positions(z, N):
    """new[b, k] = (z[b, 12k + 7], z[b, 12k + 8])"""
    xi = z[:, :12 * (N + 1)].reshape(z.shape[0], N + 1, 12)
    return xi[:, :, 7:9].copy()


def planted_agent(B):
    """The agent a plant goes to: agent 2 (close by its move) where there is one, else the last."""
    return 2 if B >= 3 else B - 1


def publish_instance(shape, plant="plain", seed=11):
    """Random z; the exchange buffer's local rows are the predicted positions moved by up to 0.05 (agents b with
    b % 3 == 1: not close under atol = 0.01) or 0.005 (the others: close).  ``plant`` puts one non-finite value
    into agent ``planted_agent(B)``: a NaN in z's very last entry, +inf in a slack entry (12 k + 10, k = N), -inf in
    a u entry, or a NaN / an inf in prev's LAST entries (index 2N+1 / 2N: past one pass of the wave where 2(N+1) >
    64).  Returns (z, traj_all, status, self_offset)."""
    N, B, n, off = shape
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, nz_of(N)))
    traj = rng.standard_normal((n, N + 1, 2))
    move = np.where(np.arange(B) % 3 == 1, 0.05, 0.005)[:, None, None]
    step = move * rng.uniform(-1.0, 1.0, (B, N + 1, 2))
    step[:, 0, 0] = move[:, 0, 0]                           # the full move somewhere: an odd agent IS not close
    traj[off:off + B] = positions(z, N) + step
    t = planted_agent(B)
    if plant == "z_last_nan":
        z[t, -1] = np.nan
    elif plant == "slack_inf":
        z[t, 12 * N + 10] = np.inf
    elif plant == "u_neg_inf":
        z[t, 12 * (N + 1) + 1] = -np.inf
    elif plant == "prev_nan":
        traj[off + t, N, 1] = np.nan
    elif plant == "prev_inf":
        traj[off + t, N, 0] = np.inf
    elif plant != "plain":
        raise ValueError(plant)
    status = np.array([STATUSES[(b + off) % len(STATUSES)] for b in range(B)], np.int32)
    return z, traj, status, off


ATOL_T, GRID = 2.0 ** -7, 2.0 ** -10


def threshold_instance(shape, seed=12):
    """rtol = 0, atol = 2^-7, positions on a 2^-10 grid (every difference below is exact in fp64): every agent
    predicts prev + atol in every entry, which is close (|prev - new| == atol), and an odd agent predicts one grid
    step more in its last entry, which is not.  Returns (z, traj_all, status, self_offset)."""
    N, B, n, off = shape
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, nz_of(N)))
    traj = rng.integers(-4096, 4096, (n, N + 1, 2)) * GRID
    new = traj[off:off + B] + ATOL_T
    new[1::2, N, 1] += GRID
    for k in range(N + 1):
        z[:, 12 * k + 7], z[:, 12 * k + 8] = new[:, k, 0], new[:, k, 1]
    return z, traj, np.ones(B, np.int32), off


# ---- the captured reference cases ----

def golden_case(name):
    """The step-0 state of a captured reference run (tests/golden/<name>.npz): dict of N, dt, vx_ref, n, steps and
    the population arrays x0 (n, 9), x_last (n, N+1, 9), u_last (n, N, 2), u_old (n, 2), traj (n, N+1, 2), nbr
    (n, n-1): all other agents, in index order."""
    from oracle import lpv_ref as L

    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    n = int(d["n_agents"])
    sel = sorted([j for j in range(len(d["step"])) if d["step"][j] == 0], key=lambda j: d["agent"][j])
    return dict(N=int(d["N"]), dt=float(d["dt"]), vx_ref=float(d["vx_ref"]), n=n, steps=int(d["steps"]),
                x0=d["x0"][sel].copy(), x_last=np.stack([d[f"x_last_{j}"] for j in sel]),
                u_last=np.stack([d[f"u_last_{j}"] for j in sel]), u_old=d["u_old"][sel].copy(),
                traj=d["pose"][sel].copy(), nbr=np.array(L.neighbour_lists(n), np.int32).reshape(n, n - 1))


def handle_args(case, ctx):
    """(bp, args, kw) of cmpc.rounds.LPVRounds / LPVRoundsHandle for a ``golden_case``."""
    import cmpc
    from oracle import lpv_ref as L

    g = L.paper_gains()
    bp = cmpc.PlannerLPVBatch(g["Q"], g["Qs"], g["R"], g["dR"], case["N"], case["dt"], L.Track.build("Highway"),
                              g["wq"], L.SCALED_CAR_MODEL, L.scaled_car_limits(case["vx_ref"]), ctx=ctx)
    args = (case["x0"].copy(), case["x_last"].copy(), case["u_last"].copy(), case["nbr"].copy())
    return bp, args, dict(u_old=case["u_old"].copy(), traj=case["traj"].copy())


# ---- a consensus step on the CPU ----

def oracle_problems(case, x0, x_lin, u_lin, u_old, traj):
    """Every agent's structured QP, linearised about (x_lin, u_lin), planes and weights cut against ``traj``."""
    from oracle import lpv_ref as L

    N, dt, nbr = case["N"], case["dt"], case["nbr"]
    track, gains, lim = L.Track.build("Highway"), L.paper_gains(), L.scaled_car_limits(case["vx_ref"])
    probs = []
    for b in range(x0.shape[0]):
        if nbr.shape[1]:
            xa = np.swapaxes(traj[nbr[b]], 0, 1)             # (N+1, nb, 2)
            planes = L.compute_hyperplane(xa, traj[b], N, keep_sign=True)
            weights, _ = L.compute_weights(traj[b], xa, lim["min_dist"])
        else:
            planes, weights = np.zeros((N, 3, 0)), np.ones((N, 0))
        A, B, ey = L.estimate_abc(x_lin[b], u_lin[b], N, dt, L.SCALED_CAR_MODEL, track)
        qp = L.LPVQP(None, None, None, None, None, planes, A, B, ey, weights)
        probs.append(L.structured(qp, x0[b], u_old[b], N, lim, gains))
    return L.stack(probs)


def oracle_state(case):
    return {k: case[k].copy() for k in ("x0", "x_last", "u_last", "u_old", "traj")}


def oracle_step(case, st, rule="fixed", relax=1.0, co=DEFAULTS):
    """One consensus step on the CPU from the state ``st`` (``oracle_state``), which is advanced in place.
    ``rule`` "fixed": the step's rule — every inner round linearises about st's x_last / u_last (the previous
    step's prediction) and only the planes and weights follow the newly published positions; "relin": each inner
    round also moves the linearisation point towards its own prediction at the fixed x0, x_lin <- x_lin + relax
    (xPred - x_lin), u_lin likewise (relax = 1: x_last <- xPred, u_last <- uPred).  Returns dict(trace, agreed,
    deltas: the per-agent delta of every inner round, zs: every inner round's z, status: the last round's)."""
    from oracle import cmpc_oracle as CO

    N = case["N"]
    base = 12 * (N + 1)
    x_lin, u_lin, traj = st["x_last"], st["u_last"], st["traj"]
    trace, deltas, zs = [], [], []
    while True:
        P = oracle_problems(case, st["x0"], x_lin, u_lin, st["u_old"], traj)
        z, _, _, status = CO.solve_batch_rescue(P, nthreads=1)
        traj, _, delta, not_close, _ = S.lpv_publish(z, N, traj, status, co["atol"], co["rtol"])
        trace.append(not_close)
        deltas.append(delta)
        zs.append(z)
        stop, agreed = S.consensus_stop(trace, co["min_rounds"], co["need"], co["max_rounds"])
        if stop:
            break
        if rule == "relin":
            xp = z[:, :base].reshape(-1, N + 1, 12)[:, :x_lin.shape[1], :9]
            up = z[:, base:base + 2 * N].reshape(-1, N, 2)
            x_lin, u_lin = x_lin + relax * (xp - x_lin), u_lin + relax * (up - u_lin)
    xp = z[:, :base].reshape(-1, N + 1, 12)[:, :, :9]
    up = z[:, base:base + 2 * N].reshape(-1, N, 2)
    ok = np.isfinite(z).all(axis=1)
    if ok.all():                                             # (the captured cases stay finite)
        st.update(x0=xp[:, 1].copy(), x_last=xp[:, 1:].copy(), u_last=up.copy(), u_old=up[:, 0].copy())
    st["traj"] = traj
    return dict(trace=trace, agreed=agreed, deltas=deltas, zs=zs, status=status)
