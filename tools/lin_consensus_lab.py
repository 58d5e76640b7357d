"""Cost of the consensus step (cmpc_lin_publish_dev, cmpc_lin_rounds_step_consensus) recorded in DESIGN.md §4.

  python tools/lin_consensus_lab.py OUT.json
      The cfg3 population (1024 agents, N = 30, nx = 4, mo = 4, nb = 2) in the linear-model family
      (scenarios.lin_of_di).
      1. Launch time of cmpc_lin_publish_dev (with close, delta and the count) beside cmpc_lin_advance_dev on the z of
         the population's fifth plain round against the initial exchange buffer (every agent has moved: each adds to
         the count), and the same launch with atol = +inf (no agent adds to it); one prebuilt C call per launch, by
         HIP events around windows of 300 back-to-back launches after 10 warm-up launches, the three alternating,
         7 windows each: median and [min, max] of the per-launch time.
      2. Host wall time of one consensus step of exactly k inner rounds (min_rounds = max_rounds = k) beside k plain
         cmpc_lin_rounds_step(h, 1) calls on a twin handle, k = 1, 3, 4.  Before every timed unit both handles are
         put back to the initial state and exchange buffer (untimed), so both solve from the same start; 10 warm-up
         units, then 7 alternated windows of 10 units each: median and [min, max] of the per-unit time.  The
         difference is the publish launch plus one 4-byte read-back and stream wait per inner round, against one
         wait per plain step.
"""
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colaborativempc-_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cmpc import _lib as L  # noqa: E402
from cmpc import scenarios as S  # noqa: E402
from cmpc.rounds import LinRoundsHandle, _lin_params  # noqa: E402
from cmpc.solver import _tptr  # noqa: E402

LAUNCHES, WARMUP, WINDOWS, UNITS = 300, 10, 7, 10


def _window(fn):
    """us per launch of LAUNCHES back-to-back launches between one pair of events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / LAUNCHES


def _stats(us):
    return {"median_us": float(np.median(us)), "min_us": float(min(us)), "max_us": float(max(us)), "windows": len(us)}


def main(out):
    n, N = 1024, 30
    sc = S.make_di(n, N, 2, 2)
    sh, lin = sc.shared, S.lin_of_di(sc)
    nx, nu, ns = sh["nx"], sh["nu"], sh["ns"]
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")   # noqa: E731
    F = LinRoundsHandle.of_di(sc, log=5)                     # five plain rounds: a z, and the solver launch's time
    assert F.step(5) == 5
    z = dev(F.read()["z"])
    solver = float(np.median(F.log()["solve_ms"])) * 1e3
    F.close()
    H, P = LinRoundsHandle.of_di(sc), LinRoundsHandle.of_di(sc)
    res = {"agents": n, "N": N, "nx": nx, "nu": nu, "ns": ns, "mo": 4, "nb": 2, "launches_per_window": LAUNCHES,
           "warmup": WARMUP, "units_per_window": UNITS, "solver_launch_median_us": solver}

    # 1. the two launches
    ctx = H.ctx
    prm, dims = _lin_params(lin["prm"]), L.cmpc_lin_dims(n, N, 0, 0, nx, 0)
    traj_all, tl, x0, up = dev(sc.traj), dev(sc.traj), dev(sc.x0), dev(sc.u_prev)
    close, delta = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    pargs = (ctx.h, ct.byref(prm), ct.byref(dims), ns, nu, _tptr(z), _tptr(traj_all), 0.01, 1e-5, _tptr(tl),
             _tptr(close), _tptr(delta), _tptr(cnt), st)
    aargs = (ctx.h, ct.byref(prm), ct.byref(dims), ns, nu, _tptr(z), _tptr(x0), _tptr(up), _tptr(tl), st)
    # the same launch with atol = +inf: every agent is close, so no lane adds to the count
    qargs = pargs[:7] + (float("inf"), 0.0) + pargs[9:]
    publish = lambda: ctx.lib.cmpc_lin_publish_dev(*pargs)                                                # noqa: E731
    publish_close = lambda: ctx.lib.cmpc_lin_publish_dev(*qargs)                                          # noqa: E731
    advance = lambda: ctx.lib.cmpc_lin_advance_dev(*aargs)                                                # noqa: E731
    counted = []
    for fn in (publish, publish_close, advance):
        cnt.zero_()
        for _ in range(WARMUP):
            assert fn() == L.CMPC_OK
        counted.append(int(cnt.item()) // WARMUP)
    us = {"publish": [], "publish_close": [], "advance": []}
    for _ in range(WINDOWS):
        us["advance"].append(_window(advance))
        us["publish"].append(_window(publish))
        us["publish_close"].append(_window(publish_close))
    res["launch"] = {"lin_advance_dev": _stats(us["advance"]),
                     "lin_publish_dev": dict(_stats(us["publish"]), agents_counted=counted[0]),
                     "lin_publish_dev_all_close": dict(_stats(us["publish_close"]), agents_counted=counted[1])}
    print("launch", json.dumps(res["launch"]), flush=True)

    # 2. a consensus step of k inner rounds beside k plain steps
    def reset(h):
        h.set_state(sc.x0, sc.u_prev)
        h.set_traj(sc.traj)

    def unit(h, fn):
        reset(h)
        t0 = time.perf_counter()
        fn()
        return 1e6 * (time.perf_counter() - t0)

    res["steps"] = {}
    for k in (1, 3, 4):
        cons = lambda: H.step_consensus(1, min_rounds=k, need=1, max_rounds=k)                            # noqa: E731
        plain = lambda: [P.step(1) for _ in range(k)]                                                      # noqa: E731
        for _ in range(WARMUP):
            assert unit(H, cons) > 0 and H.consensus()["inner_rounds"] == k
            unit(P, plain)
        us = {"consensus": [], "plain": []}
        for _ in range(WINDOWS):
            us["plain"].append(sum(unit(P, plain) for _ in range(UNITS)) / UNITS)
            us["consensus"].append(sum(unit(H, cons) for _ in range(UNITS)) / UNITS)
        rec = {"consensus_step": _stats(us["consensus"]), "plain_steps": _stats(us["plain"]),
               "not_close": H.consensus()["not_close"].tolist()}
        rec["extra_us_per_inner_round"] = (rec["consensus_step"]["median_us"] - rec["plain_steps"]["median_us"]) / k
        rec["ratio"] = rec["consensus_step"]["median_us"] / rec["plain_steps"]["median_us"]
        res["steps"][f"k{k}"] = rec
        print("k", k, json.dumps(rec), flush=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
