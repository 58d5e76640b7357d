"""Launch time of the stage-table builder (cmpc_lin_table_build_dev, csrc/lin_build.hip) recorded in DESIGN.md §4.

  python tools/lin_table_lab.py OUT.json
      The cfg3 population (1024 agents, N = 30, nx = 4, mo = 4, nb = 2) as a stage table of T = 130 equal rows
      (scenarios.lin_table_of_di), windows at t = 0, 50 (inside the table) and 120 (straddling its end), HOLD and
      PERIODIC: cmpc_lin_table_build_dev beside the fixed-window cmpc_lin_build_dev on the same agents, one
      prebuilt C call per launch, by HIP events around windows of 300 back-to-back launches after 10 warm-up
      launches, the two alternating, 7 windows each: median and [min, max] of the per-launch time; and beside the
      solver launch of a round of that population (DIRounds(fused=False).step timer: median over 15 rounds after
      5), the launch the build precedes.
"""
import ctypes as ct
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colaborativempc-_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cmpc import _lib as L  # noqa: E402
from cmpc import scenarios as S  # noqa: E402
from cmpc.rounds import DIRounds, _lin_args, _lin_params, _lin_table_args, lin_build_dev, lin_table_build_dev  # noqa: E402
from cmpc.solver import _tptr  # noqa: E402

LAUNCHES, WARMUP, WINDOWS = 300, 10, 7


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
    n, N, T = 1024, 30, 130
    sc = S.make_di(n, N, 2, 2)
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")   # noqa: E731
    lin, tl = S.lin_of_di(sc), S.lin_table_of_di(sc, T)
    own = {k: dev(v) for k, v in lin["own"].items()}
    table = {k: dev(v) for k, v in tl["table"].items()}
    nbr, traj = dev(sc.nbr, torch.int32), dev(sc.traj)
    R = DIRounds(sc, fused=False)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for e in ev:
        R.step(timer=e)
    torch.cuda.synchronize()
    solver = float(np.median([1e3 * a.elapsed_time(b) for a, b in ev[5:]]))
    prm = _lin_params(lin["prm"])
    # the fixed-window builder: the wrapper once (it allocates the outputs), then the C call alone
    fixed_out = lin_build_dev(lin["prm"], own, nbr, traj)
    ctx, fd, lo, pn, st = _lin_args(traj, nbr, own, 0, None, None)
    fargs = (ctx.h, ct.byref(prm), ct.byref(fd), pn, ct.byref(lo), _tptr(traj), *[_tptr(o) for o in fixed_out], st)
    fixed = lambda: ctx.lib.cmpc_lin_build_dev(*fargs)                                                    # noqa: E731
    res = {"agents": n, "N": N, "T": T, "nx": 4, "nu": 2, "mo": 4, "nb": 2, "launches_per_window": LAUNCHES,
           "warmup_launches": WARMUP, "solver_launch_median_us": solver,
           "window_bytes_A_B": 8 * n * N * (4 * 4 + 4 * 2), "cases": {}}
    for mode, name in ((L.CMPC_TABLE_HOLD, "hold"), (L.CMPC_TABLE_PERIODIC, "periodic")):
        for t in (0, 50, 120):
            tab_out = lin_table_build_dev(tl["prm"], table, t, N, nbr, traj, mode)
            ctx, td_, nu, tdims, tab, pn, st = _lin_table_args(table, N, nbr, traj, mode, 0, None, None)
            targs = (ctx.h, ct.byref(prm), ct.byref(td_), nu, ct.byref(tdims), ct.byref(tab), t, pn, _tptr(traj),
                     *[_tptr(o) for o in tab_out], st)
            tabf = lambda: ctx.lib.cmpc_lin_table_build_dev(*targs)                                       # noqa: E731
            for fn in (fixed, tabf):
                for _ in range(WARMUP):
                    assert fn() == L.CMPC_OK
            torch.cuda.synchronize()
            us = {"fixed": [], "table": []}
            for _ in range(WINDOWS):                                                                       # alternating
                us["fixed"].append(_window(fixed))
                us["table"].append(_window(tabf))
            # equal rows: the table's build is the fixed window's, and its windows are the scenario's A, B
            same = all(torch.equal(a, b) for a, b in zip(tab_out[2:], fixed_out)) and \
                torch.equal(tab_out[0], dev(sc.A)) and torch.equal(tab_out[1], dev(sc.B))
            rec = {"lin_build_dev": _stats(us["fixed"]), "lin_table_build_dev": _stats(us["table"]),
                   "identical_outputs": bool(same)}
            rec["ratio_table_to_fixed"] = rec["lin_table_build_dev"]["median_us"] / rec["lin_build_dev"]["median_us"]
            rec["share_of_solver_launch"] = rec["lin_table_build_dev"]["median_us"] / solver
            res["cases"][f"{name}_t{t}"] = rec
            print(name, t, json.dumps(rec), flush=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
