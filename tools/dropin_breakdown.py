"""Where the time of one literal ``osqp_solve_qp`` call goes (test infrastructure; GPU box).

bench.py's `osqp_dropin` line times the whole call on the 12 reference-captured N = 30 agent QPs of
tests/golden/lpv_n30_a3.npz.  This splits it into the host-side structure recognition
(cmpc.structure.recognize), the structured solve (cmpc.solver.solve_mpc with the rescue + polish
policy: host -> HBM copies, the launches, HBM -> host) and the OSQP-style result (objective, primal
residual), per QP, mean over `reps` passes.

  python tools/dropin_breakdown.py [reps] [--lpv-structure] [--detector]

--lpv-structure: the adapter and the structured solve run with the reference structure detected on the device
(osqp_solve_qp(lpv_structure=True), solve_mpc(lpv="auto")): the condensed kernel's compact instantiation.
--detector: also time cmpc_mpc_lpv_level_dev alone on the 12 QPs tiled to 1024 agents (device arrays, events
around each of 200 launches after 20 warm-up launches; median and minimum).
"""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colaborativempc-_amd")]


def qps_of_golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "lpv_n30_a3.npz"), allow_pickle=False)

    def mat(nm, j):
        shp = tuple(int(v) for v in d[f"{nm}_{j}_shape"])
        return sp.csr_matrix((d[f"{nm}_{j}_data"], (d[f"{nm}_{j}_row"], d[f"{nm}_{j}_col"])), shape=shp)

    qps = []
    for j in range(len(d["step"])):
        Aall, l, u = mat("A", j), d["l"][j], d["u"][j]
        eq = np.isfinite(l) & (l == u)
        qps.append((mat("P", j), d["q"][j], Aall[np.flatnonzero(~eq)], u[~eq], Aall[np.flatnonzero(eq)], u[eq]))
    return qps, d["z"]


def detector_us(ctx, probs, agents=1024, reps=200):
    import ctypes as ct

    import torch

    from cmpc import _lib as L
    from cmpc import structure as St
    from cmpc.solver import _dims, _tptr, _weights

    p = St.stack(probs)
    idx = np.arange(agents) % p["A"].shape[0]
    dev = torch.device("cuda", ctx.device)
    t = {k: torch.as_tensor(np.ascontiguousarray(p[k][idx]), device=dev) for k in ("A", "B", "C")}
    lv = torch.zeros(agents, dtype=torch.int32, device=dev)
    nc = torch.zeros(1, dtype=torch.int32, device=dev)
    w, keep = _weights(p)
    data = L.cmpc_mpc_data(_tptr(t["A"]), _tptr(t["B"]), None, None, None, _tptr(t["C"]), None)
    d = _dims(p, agents)
    s = torch.cuda.current_stream(dev)
    times = []
    for i in range(reps + 20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        ctx.check(ctx.lib.cmpc_mpc_lpv_level_dev(ctx.h, ct.byref(d), ct.byref(w), ct.byref(data), _tptr(lv), _tptr(nc),
                                                 ct.c_void_p(s.cuda_stream)))
        e1.record(s)
        e1.synchronize()
        if i >= 20:
            times.append(e0.elapsed_time(e1) * 1e3)
    assert int(nc.cpu()[0]) == 0 and bool((lv == 2).all())
    mb = sum(v.numel() for v in t.values()) * 8 / 1e6
    return dict(agents=agents, N=int(p["N"]), mc=int(p["mc"]), mbytes=round(mb, 2),
                median_us=round(float(np.median(times)), 2), min_us=round(float(np.min(times)), 2))


def main(reps, lpv_structure=False, detector=False):
    import cmpc
    from cmpc import qp as Q
    from cmpc import structure as St
    from cmpc.solver import solve_mpc

    ctx = cmpc.default_context() if hasattr(cmpc, "default_context") else None
    qps, zc = qps_of_golden()
    t_rec, t_sol, t_res, t_all, iters = [], [], [], [], []
    for rep in range(reps + 1):
        for j, (P, q, G, h, A, b) in enumerate(qps):
            t0 = time.perf_counter()
            p = St.recognize(P, q, G, h, A, b)
            t1 = time.perf_counter()
            z, kkt, it, st = solve_mpc(St.stack([p]), ctx, rescue=True, polish=True,
                                       lpv="auto" if lpv_structure else False)
            t2 = time.perf_counter()
            x = z[0]
            Q._osqp_result(x, None, int(st[0]), "solved", int(it[0]), float(0.5 * x @ (P @ x) + q @ x), float(kkt[0]),
                           Q._pri_res(x, G, h, A, b), float("nan"), "structured")
            t3 = time.perf_counter()
            cmpc.osqp_solve_qp(P, q, G, h, A, b, ctx=ctx, lpv_structure=lpv_structure)
            t4 = time.perf_counter()
            if rep:   # the first pass warms up
                t_rec.append(t1 - t0)
                t_sol.append(t2 - t1)
                t_res.append(t3 - t2)
                t_all.append(t4 - t3)
                iters.append(int(it[0]))
            assert np.abs(x - zc[j]).max() < 1e-6
    ms = lambda v: round(float(np.mean(v)) * 1e3, 4)  # noqa: E731
    out = {"detector": detector_us(ctx, [St.recognize(*qp) for qp in qps])} if detector else {}
    print(json.dumps({"qps": len(qps), "reps": reps, "lpv_structure": bool(lpv_structure), **out, "recognize_ms": ms(t_rec), "solve_ms": ms(t_sol),
                      "result_ms": ms(t_res), "osqp_solve_qp_ms": ms(t_all),
                      "solve_ms_max": round(float(np.max(t_sol)) * 1e3, 4),
                      "iters": sorted(set(iters))}))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(int(args[0]) if args else 20, "--lpv-structure" in sys.argv, "--detector" in sys.argv)
