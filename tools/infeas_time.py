"""Launch time of the infeasibility-certificate kernels (csrc/mpc_infeas.hip, csrc/mpc_infeas_rows.hip) beside a
solver launch, on the GPU.

Device-resident synthetic batch (scenarios.make_di: nx = 4, nu = 2, mc = 6), HIP events around windows of
launches, the variants alternated:

  solve          cmpc_solve_mpc_batch_dev
  solve+flag     the same with CMPC_FLAG_CERTIFY (every agent solved: each certificate wavefront returns at once)
  certify        cmpc_mpc_certify_dev alone with status = NULL: every agent examined, no ray written
  solve+rows     the solve with CMPC_FLAG_CERTIFY | CMPC_FLAG_CERTIFY_ROWS (every agent solved: both certificate
                 launches return at once: the cost the flags add to a healthy round)
  rows           cmpc_mpc_certify_rows_dev alone with status = NULL and the defaults: every agent examined; a
                 feasible agent stops at its first check (8 iterations)
  rows_cap       the same with max_iter = check_every = CMPC_CERT_ROWS_MAX_ITER: every agent runs to the cap
                 (a tenth of the calls per window)

Prints one JSON line: the median microseconds per call of each variant and the windows' spread.

    python tools/infeas_time.py [--agents 1024] [--N 30] [--calls 300] [--windows 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colaborativempc-_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()

    import torch

    import cmpc
    from cmpc import infeas
    from cmpc import scenarios as S
    from oracle import synth

    ctx = cmpc.default_context(0)
    dev = torch.device("cuda", 0)
    sc = S.make_di(a.agents, a.N, 2, 2)
    P = synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj,
                         np.arange(a.agents))
    d = {k: torch.from_numpy(np.ascontiguousarray(P[k], dtype=np.float64)).to(dev) for k in cmpc.solver.PER_AGENT}
    out = dict(z=torch.zeros((a.agents, cmpc.nz_of(P)), dtype=torch.float64, device=dev),
               kkt=torch.zeros(a.agents, dtype=torch.float64, device=dev),
               iters=torch.zeros(a.agents, dtype=torch.int32, device=dev),
               status=torch.zeros(a.agents, dtype=torch.int32, device=dev))
    margin = torch.zeros(a.agents, dtype=torch.float64, device=dev)
    row = torch.zeros(a.agents, dtype=torch.int32, device=dev)
    its = torch.zeros(a.agents, dtype=torch.int32, device=dev)
    cap = infeas.CERT_ROWS_MAX_ITER
    variants = {"solve": lambda: cmpc.solve_mpc_dev(P, d, out, ctx),
                "solve+flag": lambda: cmpc.solve_mpc_dev(P, d, out, ctx, certify=True),
                "certify": lambda: infeas.certify_dev(P, d, None, None, margin, row, ctx=ctx),
                "solve+rows": lambda: cmpc.solve_mpc_dev(P, d, out, ctx, certify="rows"),
                "rows": lambda: infeas.certify_rows_dev(P, d, None, None, margin, its, ctx=ctx),
                "rows_cap": lambda: infeas.certify_rows_dev(P, d, None, None, margin, its, max_iter=cap,
                                                            check_every=cap, ctx=ctx)}
    calls = {k: max(1, a.calls // 10) if k == "rows_cap" else a.calls for k in variants}
    for k, f in variants.items():
        for _ in range(10 if calls[k] == a.calls else 1):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.windows):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[k]):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(1e3 * e0.elapsed_time(e1) / calls[k])
    st = out["status"].cpu().numpy()
    res = dict(agents=a.agents, N=a.N, calls=a.calls, windows=a.windows, solved=int((st == 1).sum()),
               iters_max=int(out["iters"].max()), certified=int((row.cpu().numpy() >= 0).sum()), rows_cap_iters=int(its.min()))
    for k, v in times.items():
        res[k + "_us"] = round(float(np.median(v)), 1)
        res[k + "_spread"] = round(float((max(v) - min(v)) / np.median(v)), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
