"""What CMPC_FLAG_LPV_SPLIT costs and gains (test infrastructure; GPU box).

The 12 reference-captured N = 30 agent QPs of tests/golden/lpv_n30_a3.npz as one structured batch, and tiled to 1024
agents, on the device entry (cmpc_solve_mpc_batch_dev, no rescue: the solver launches alone).  HIP events around each
call, 10 warm-up and 200 timed calls per variant, the variants alternated call by call in one process; median and
minimum in microseconds.

  all conforming   promise (one launch, CMPC_FLAG_LPV) against split (four launches): the difference is the detector,
                   the partition and an empty launch
  mixed            1024 agents with 0, 10, 50 and 100 % of them moved off the pattern (B's row 3 at every stage):
                   split against plain (what CMPC_FLAG_LPV_AUTO gives such a batch) and, at 0 %, against the promise

  python tools/lpv_split_lab.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colaborativempc-_amd"), os.path.join(ROOT, "tools")]

WARM, REPS = 10, 200


def batch_of(agents, planted_frac=0.0, seed=0):
    from cmpc import structure as St
    from cmpc.solver import PER_AGENT
    from dropin_breakdown import qps_of_golden

    qps, _ = qps_of_golden()
    p = St.stack([St.recognize(*qp) for qp in qps])
    idx = np.arange(agents) % p["A"].shape[0]
    out = dict(p)
    for k in PER_AGENT:
        out[k] = np.ascontiguousarray(p[k][idx])
    n = int(round(planted_frac * agents))
    if n:
        hit = np.random.default_rng(seed).choice(agents, size=n, replace=False)
        out["B"][hit, :, 3, 0] = 0.5
    return out, n


def timed(ctx, p, variants):
    """{name: (median_us, min_us)} of solve_mpc_dev under each variant's lpv argument, alternated call by call."""
    import torch

    from cmpc.solver import PER_AGENT, nz_of, solve_mpc_dev

    dev = torch.device("cuda", ctx.device)
    batch = p["A"].shape[0]
    t = {k: torch.as_tensor(np.ascontiguousarray(p[k], dtype=np.float64), device=dev) for k in PER_AGENT}
    out = dict(z=torch.zeros((batch, nz_of(p)), dtype=torch.float64, device=dev),
               kkt=torch.zeros(batch, dtype=torch.float64, device=dev),
               iters=torch.zeros(batch, dtype=torch.int32, device=dev),
               status=torch.zeros(batch, dtype=torch.int32, device=dev))
    s = torch.cuda.current_stream(dev)
    times = {k: [] for k in variants}
    iters = {}
    for i in range(WARM + REPS):
        for name, lpv in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            solve_mpc_dev(p, t, out, ctx, lpv=lpv)
            e1.record(s)
            e1.synchronize()
            if i >= WARM:
                times[name].append(e0.elapsed_time(e1) * 1e3)
            elif i == 0:
                iters[name] = int(out["iters"].max().cpu())
    return {k: dict(median_us=round(float(np.median(v)), 1), min_us=round(float(np.min(v)), 1), max_iters=iters[k])
            for k, v in times.items()}


def main(path=None):
    import cmpc

    ctx = cmpc.default_context()
    res = {"warmup": WARM, "reps": REPS, "entry": "cmpc_solve_mpc_batch_dev, no rescue", "all_conforming": {}, "mixed": {}}
    for agents in (12, 1024):
        p, _ = batch_of(agents)
        r = timed(ctx, p, {"promise": True, "split": "split"})
        r["split_minus_promise_us"] = round(r["split"]["median_us"] - r["promise"]["median_us"], 1)
        res["all_conforming"][str(agents)] = r
    for frac in (0.0, 0.1, 0.5, 1.0):
        p, n = batch_of(1024, frac, seed=7)
        variants = {"plain": False, "split": "split"}
        if n == 0:
            variants["promise"] = True
        r = timed(ctx, p, variants)
        r["planted"] = n
        r["plain_over_split"] = round(r["plain"]["median_us"] / r["split"]["median_us"], 3)
        res["mixed"][f"{int(frac * 100)}%"] = r
    text = json.dumps(res, indent=1)
    print(text)
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
