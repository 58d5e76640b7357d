"""Measurements of the device launch order (csrc/order.hip) and of the synthetic family's round handle
(cmpc_di_rounds_*) recorded in DESIGN.md §4.

  python tools/order_lab.py time OUT.json
      launch time of cmpc_order_by_iters_dev by HIP events (10 warm-up launches, 200 timed one by one: median
      and range; and 200 back to back between one pair of events) on a round's real iteration counts at 1024
      agents (cfg3: N = 30, 2-D) and 8192 agents (cfg5: N = 50, 3-D), beside the torch.argsort(descending,
      stable) + .to(int32) it replaces, timed the same way in the same run (alternating), and beside the solver
      launch of a round of that population (DIRounds.step timer: median over 15 rounds after 5).
  python tools/order_lab.py rounds OUT.json [repeats] [rounds]
      cfg5-shaped rounds (8192 agents, N = 50, 3-D, nb = 2): ms per round of the handle with CMPC_ROUNDS_LPT off
      and on and of DIRounds(lpt=True), each `repeats` times `rounds` rounds after 5 warm-up rounds, the three
      alternating (host clock around work that ends in a device synchronise); the spread over the repeats.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colaborativempc-_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cmpc import scenarios as S  # noqa: E402
from cmpc.rounds import DIRounds, DIRoundsHandle, order_by_iters_dev  # noqa: E402


def _events(n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def _stats(ms):
    ms = np.asarray(ms)
    return {"median_us": 1e3 * float(np.median(ms)), "min_us": 1e3 * float(ms.min()), "max_us": 1e3 * float(ms.max()),
            "n": int(ms.size)}


def _time(fn, n=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev = _events(n)
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    one = _stats([a.elapsed_time(b) for a, b in ev])
    a, b = _events(1)[0]
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    one["back_to_back_us"] = 1e3 * a.elapsed_time(b) / n
    return one


def time_order(out):
    res = {}
    for name, (n, N, dim) in (("cfg3", (1024, 30, 2)), ("cfg5", (8192, 50, 3))):
        R = DIRounds(S.make_di(n, N, 2, dim))
        ev = _events(20)
        for e in ev:
            R.step(timer=e)
        torch.cuda.synchronize()
        it = R.iters.clone()
        rec = {"agents": n, "N": N, "dim": dim, "lpt": bool(R.lpt),
               "iters_min_max": [int(it.min()), int(it.max())],
               "solver_launch": _stats([a.elapsed_time(b) for a, b in ev[5:]])}
        order = torch.empty(n, dtype=torch.int32, device="cuda")
        dev = lambda: order_by_iters_dev(it, out=order)                                          # noqa: E731
        tor = lambda: torch.argsort(it, descending=True, stable=True).to(torch.int32)            # noqa: E731
        passes = [(_time(dev), _time(tor)) for _ in range(3)]                                    # alternating
        assert np.array_equal(order.cpu().numpy(), S.order_by_iters(it.cpu().numpy()))
        assert torch.equal(order, tor())
        rec["order_kernel"] = [p[0] for p in passes]
        rec["torch_argsort_to_int32"] = [p[1] for p in passes]
        med = float(np.median([p[0]["median_us"] for p in passes]))
        rec["order_kernel_median_us"] = med
        rec["torch_median_us"] = float(np.median([p[1]["median_us"] for p in passes]))
        rec["share_of_solver_launch"] = med / rec["solver_launch"]["median_us"]
        res[name] = rec
        print(name, json.dumps(rec), flush=True)
    json.dump(res, open(out, "w"), indent=1)


def time_rounds(out, repeats=4, rounds=20):
    sc = S.make_di(8192, 50, 2, 3)
    runs = {"handle_lpt_off": DIRoundsHandle(sc, lpt=False), "handle_lpt_on": DIRoundsHandle(sc, lpt=True),
            "dirounds_lpt_on": DIRounds(sc, lpt=True)}

    def go(name, k):
        r = runs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name.startswith("handle"):
            r.step(k)                      # synchronises once, at the end
        else:
            for _ in range(k):
                r.step()
            torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    for name in runs:
        go(name, 5)
    ms = {name: [] for name in runs}
    for _ in range(repeats):
        for name in runs:
            ms[name].append(go(name, rounds))
    # the three ran the same rounds of the same population: the same results
    a, b = runs["handle_lpt_off"].read(), runs["handle_lpt_on"].read()
    R = runs["dirounds_lpt_on"]
    same = all(a[k].tobytes() == b[k].tobytes() for k in a) and a["z"].tobytes() == R.z.cpu().numpy().tobytes()
    res = {"agents": 8192, "N": 50, "dim": 3, "nb": 2, "warmup_rounds": 5, "rounds_per_repeat": rounds,
           "ms_per_round": ms, "identical_outputs": bool(same),
           "median_ms_per_round": {k: float(np.median(v)) for k, v in ms.items()},
           "spread_ms_per_round": {k: [float(min(v)), float(max(v))] for k, v in ms.items()}}
    print(json.dumps(res), flush=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "time":
        time_order(sys.argv[2])
    else:
        time_rounds(sys.argv[2], *(int(a) for a in sys.argv[3:5]))
