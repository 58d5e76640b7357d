"""What the rounds' device log costs (cmpc_*_rounds_log_*): rounds per second of the two round
handles with the log off, on, and on with CMPC_LOG_SEPARATION.

  python tools/round_log_lab.py OUT.json [repeats] [rounds] [--no-log]

  DIRoundsHandle on cfg3 (1024 agents, N = 30, 2-D, nb = 2) and LPVRoundsHandle on bench.lpv_population's 1023
  agents (N = 30, CMPC_ROUNDS_NO_HALT so that the step call ends in its one synchronise): per variant a handle of
  its own on the same population, 5 warm-up rounds, then `repeats` (5) step calls of `rounds` (100) rounds each,
  the variants alternating; host clock around the step call.  The log's capacity is `rounds`.  After the timing
  the variants' final states are compared (the log changes no result) and a log is read once (its time is given
  apart: it is not part of a step).
  --no-log: the log-off variant alone, for a build of the library from before the log (CMPC_LIB_PATH=...; its
  missing entry points are left out of the binding).  Run the two builds alternately in one session and compare
  their log-off numbers: the claim is that they differ by no more than either's own spread.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colaborativempc-_amd"))
sys.path.insert(0, ROOT)

from cmpc import _lib as L  # noqa: E402

NO_LOG = "--no-log" in sys.argv
if NO_LOG:
    for name in [k for k in L.SIGNATURES if "_log" in k]:
        del L.SIGNATURES[name]

import bench  # noqa: E402
from cmpc import scenarios as S  # noqa: E402
from cmpc.rounds import DIRoundsHandle, LPVRoundsHandle  # noqa: E402

VARIANTS = {"log_off": {}} if NO_LOG else {"log_off": {}, "log_on": dict(log=True), "log_on_separation": dict(log=True, sep=True)}


def measure(make, repeats, rounds):
    runs = {}
    for name, v in VARIANTS.items():
        kw = dict(log=rounds, log_separation=bool(v.get("sep"))) if v.get("log") else {}
        runs[name] = make(**kw)

    def go(name, k):
        t0 = time.perf_counter()
        done = runs[name].step(k)              # ends in the step's own synchronise
        dt = time.perf_counter() - t0
        assert done in (k, (k, 0)) or (isinstance(done, tuple) and done[0] == k), done
        return k / dt

    for name in runs:
        go(name, 5)
    rps = {name: [] for name in runs}
    for _ in range(repeats):
        for name in runs:
            rps[name].append(go(name, rounds))
    ref = runs["log_off"].read()
    same = all(all(r.read()[k].tobytes() == ref[k].tobytes() for k in ref) for r in runs.values())
    st = np.unique(ref["status"], return_counts=True)
    res = {"warmup_rounds": 5, "rounds_per_step_call": rounds, "repeats": repeats, "rounds_per_s": rps,
           "median_min_max_rounds_per_s": {k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in rps.items()},
           "identical_final_state": bool(same),
           "last_round_status_counts": {int(k): int(c) for k, c in zip(*st)}}
    if not NO_LOG:
        med = res["median_min_max_rounds_per_s"]
        res["log_cost_us_per_round"] = {k: 1e6 * (1 / med[k][0] - 1 / med["log_off"][0]) for k in med if k != "log_off"}
        t0 = time.perf_counter()
        lg = runs["log_on_separation"].log()
        res["log_read_ms"] = 1e3 * (time.perf_counter() - t0)
        res["log_read_rounds"] = int(len(lg["solve_ms"]))
        ms = lg["solve_ms"]
        res["solve_ms_median_min_max"] = [float(np.median(ms)), float(ms.min()), float(ms.max())]   # the last call's rounds
    for r in runs.values():
        r.close()
    return res


def main(out, repeats=5, rounds=100):
    ctx = L.default_context(0)
    res = {"library": os.path.relpath(L.LIB_PATH, ROOT), "no_log_build": NO_LOG}
    sc = S.make_di(1024, 30, 2, 2)
    res["di_cfg3"] = dict(agents=1024, N=30, dim=2, nb=2, **measure(lambda **kw: DIRoundsHandle(sc, ctx=ctx, **kw),
                                                                    repeats, rounds))
    print("di_cfg3", json.dumps(res["di_cfg3"]), flush=True)
    bp, args, kw0 = bench.lpv_population(ctx, 341)
    res["lpv_1023"] = dict(agents=int(len(args[0])), N=int(bp.N), **measure(
        lambda **kw: LPVRoundsHandle(bp, *args, **kw0, halt=False, **kw), repeats, rounds))
    print("lpv_1023", json.dumps(res["lpv_1023"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if not x.startswith("--")]
    main(a[0], *(int(x) for x in a[1:3]))
