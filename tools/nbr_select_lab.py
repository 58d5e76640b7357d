"""Measurements of the device neighbour selection (csrc/nbr_select.hip) recorded in DESIGN.md §4.

  python tools/nbr_select_lab.py time OUT.json
      launch time of cmpc_nbr_select_dev by HIP events (10 warm-up launches, 200 timed one by one: median and
      range; and 200 back to back between one pair of events) at cfg3 (1024 agents, N = 30, nb = 2) and cfg4
      (4096 agents), windows (0, 0) and (0, N), beside the round's solver launch of the same population
      (DIRounds.step timer: median over 20 rounds after 5).
  python tools/nbr_select_lab.py loop OUT.json [rounds]
      closed loop, cfg3, reselect = 0 and = 1: per round the agents whose two nearest (host selection on the
      exchange buffer the round was built from) are not both in the table the round used, and the smallest
      stage-0 distance between an agent and an agent outside its table, against min_dist.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colaborativempc-_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cmpc import scenarios as S  # noqa: E402
from cmpc.rounds import DIRounds, select_neighbours_dev  # noqa: E402


def _events(n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def _stats(ms):
    ms = np.asarray(ms)
    return {"median_us": 1e3 * float(np.median(ms)), "min_us": 1e3 * float(ms.min()), "max_us": 1e3 * float(ms.max()),
            "n": int(ms.size)}


def time_select(out):
    res = {}
    for name, n in (("cfg3", 1024), ("cfg4", 4096)):
        sc = S.make_di(n, 30, 2)
        R = DIRounds(sc)
        ev = _events(25)
        for e in ev:
            R.step(timer=e)
        torch.cuda.synchronize()
        rec = {"agents": n, "N": 30, "nb": 2,
               "solver_launch": _stats([a.elapsed_time(b) for a, b in ev[5:]])}
        nbr = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        for w in ((0, 0), (0, 30)):
            for _ in range(10):
                select_neighbours_dev(R.traj_all, 2, window=w, out=nbr)
            torch.cuda.synchronize()
            ev = _events(200)
            for a, b in ev:
                a.record()
                select_neighbours_dev(R.traj_all, 2, window=w, out=nbr)
                b.record()
            torch.cuda.synchronize()
            one = _stats([a.elapsed_time(b) for a, b in ev])
            a, b = _events(1)[0]
            a.record()
            for _ in range(200):
                select_neighbours_dev(R.traj_all, 2, window=w, out=nbr)
            b.record()
            torch.cuda.synchronize()
            one["back_to_back_us"] = 1e3 * a.elapsed_time(b) / 200
            one["pair_evaluations"] = n * n * (w[1] - w[0] + 1)
            one["share_of_solver_launch"] = one["median_us"] / rec["solver_launch"]["median_us"]
            if one["pair_evaluations"] <= 1 << 26:   # the host statement of the largest case takes a while
                assert np.array_equal(nbr.cpu().numpy(), S.select_neighbours(R.traj_all.cpu().numpy(), 2, w))
            rec[f"window_{w[0]}_{w[1]}"] = one
        res[name] = rec
        print(name, json.dumps(rec), flush=True)
    json.dump(res, open(out, "w"), indent=1)


def closed_loop(out, rounds=100):
    res = {}
    for reselect in (0, 1):
        sc = S.make_di(1024, 30, 2)
        R = DIRounds(sc, reselect=reselect)
        stale, gap, unsolved = [], [], 0
        for _ in range(rounds):
            traj = R.traj_all.cpu().numpy()
            R.step()
            torch.cuda.synchronize()
            table = R.nbr.cpu().numpy()          # the table this round was built with
            idx, d2 = S.select_neighbours(traj, 4, return_dist2=True)
            both = np.array([set(idx[g, :2]) <= set(table[g]) for g in range(1024)])
            stale.append(int((~both).sum()))
            # nearest agent outside the table: the first of the four nearest that the table does not hold
            outside = np.array([next(d for j, d in zip(idx[g], d2[g]) if j not in table[g]) for g in range(1024)])
            gap.append(float(np.sqrt(outside.min())))
            unsolved += int((R.status.cpu().numpy() != 1).sum())
        res[f"reselect_{reselect}"] = {"rounds": rounds, "agents_with_a_stale_table": stale,
                                       "min_distance_to_an_agent_outside_the_table": gap,
                                       "min_dist": sc.params["min_dist"], "agent_rounds_not_solved": unsolved}
        print(reselect, "stale", stale[::10], "gap", [round(g, 3) for g in gap[::10]], "not solved", unsolved,
              flush=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "time":
        time_select(sys.argv[2])
    else:
        closed_loop(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 100)
