"""Launch times of the 3-D position kernels (cmpc_lin3_*, cmpc_nbr_select3_dev) beside their planar namesakes,
recorded in DESIGN.md §4.

  python tools/lin3_lab.py OUT.json
      Builder, advance and publish on the 3-D double integrator (nx = 6, nu = 3, ns = 3, mo = 4, nb = 2;
      scenarios.make_di(n, N, 2, 3)) at 1024 agents, N = 30 and at 8192 agents, N = 50: the planar entry on
      lin_of_di, the 3-D entry on lin3_of_di with every agent at its own altitude.  The selector at the sizes of
      DESIGN's selector table (1024 and 4096 agents, N = 30, nb = 2), windows (0, 0) and (0, N), on the 3-column
      buffer and on its first two columns.  One prebuilt C call per launch, device-resident arguments, HIP events
      around windows of 300 back-to-back launches after 10 warm-up launches, planar and 3-D alternating, 7 windows
      each: median and [min, max] of the per-launch time in microseconds.
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
from cmpc.rounds import _lin_args, _lin_fn, _lin_params, _pos_dim, lin_build_dev  # noqa: E402
from cmpc.solver import _tptr  # noqa: E402

LAUNCHES, WARMUP, WINDOWS = 300, 10, 7


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


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


def pair(planar, three):
    """Alternating windows of the two launches; returns the record of the pair."""
    for fn in (planar, three):
        for _ in range(WARMUP):
            assert fn() == L.CMPC_OK
    torch.cuda.synchronize()
    us = {"planar": [], "three": []}
    for _ in range(WINDOWS):
        us["planar"].append(_window(planar))
        us["three"].append(_window(three))
    rec = {"planar": _stats(us["planar"]), "three_d": _stats(us["three"])}
    rec["ratio"] = rec["three_d"]["median_us"] / rec["planar"]["median_us"]
    return rec


def family(n, N):
    """Builder, advance, publish of one population: {kernel: record}."""
    sc = S.make_di(n, N, 2, 3)
    rng = np.random.default_rng(1)
    lins = (S.lin_of_di(sc), S.lin3_of_di(sc, rng.uniform(0.0, 1.0, n)))
    nx, nu, ns = 6, 3, 3
    z = dev(rng.standard_normal((n, (nx + ns) * (N + 1) + 2 * nu * N)))
    nbr = dev(sc.nbr, torch.int32)
    own = {k: dev(v) for k, v in lins[0]["own"].items()}
    calls = {"build": [], "advance": [], "publish": []}
    keep = []
    for lin in lins:
        prm, traj = lin["prm"], dev(lin["traj"])
        cp = _lin_params(prm)
        out = lin_build_dev(prm, own, nbr, traj)
        ctx, d, lo, pn, st = _lin_args(traj, nbr, own, 0, None, None, _pos_dim(prm))
        x0, up, tl = dev(sc.x0), dev(sc.u_prev), torch.zeros_like(traj)
        close, delta, cnt = (torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.float64,
                             device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
        keep.append((cp, d, lo, out, traj, x0, up, tl, close, delta, cnt))
        b = (_lin_fn(ctx, prm, "build_dev"), (ctx.h, ct.byref(cp), ct.byref(d), pn, ct.byref(lo), _tptr(traj),
                                              *[_tptr(o) for o in out], st))
        a = (_lin_fn(ctx, prm, "advance_dev"), (ctx.h, ct.byref(cp), ct.byref(d), ns, nu, _tptr(z), _tptr(x0), _tptr(up),
                                                _tptr(tl), st))
        p = (_lin_fn(ctx, prm, "publish_dev"), (ctx.h, ct.byref(cp), ct.byref(d), ns, nu, _tptr(z), _tptr(traj), 0.01,
                                                1e-5, _tptr(tl), _tptr(close), _tptr(delta), _tptr(cnt), st))
        for k, (fn, args) in zip(("build", "advance", "publish"), (b, a, p)):
            calls[k].append(lambda fn=fn, args=args: fn(*args))
    res = {k: pair(*v) for k, v in calls.items()}
    del keep
    return res


def selector(n, N, window):
    sc = S.make_di(n, N, 2, 3)
    x0 = sc.x0.copy()
    x0[:, 2] = np.random.default_rng(2).uniform(0.0, 1.0, n)
    t3 = dev(S.rollout3(x0, N))
    t2 = t3[..., :2].contiguous()
    ctx = L.default_context(0)
    st = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = L.cmpc_nbr_dims(n, N, 2, 0, n, window[0], window[1])
    o2, o3 = (torch.zeros((n, 2), dtype=torch.int32, device="cuda") for _ in range(2))
    planar = lambda: ctx.lib.cmpc_nbr_select_dev(ctx.h, ct.byref(dims), _tptr(t2), _tptr(o2), None, st)    # noqa: E731
    three = lambda: ctx.lib.cmpc_nbr_select3_dev(ctx.h, ct.byref(dims), _tptr(t3), _tptr(o3), None, st)    # noqa: E731
    rec = pair(planar, three)
    rec["pair_evaluations"] = n * (n - 1) * (window[1] - window[0] + 1)
    return rec


def main(out):
    res = {"launches_per_window": LAUNCHES, "warmup_launches": WARMUP, "family": {}, "selector": {}}
    for n, N in ((1024, 30), (8192, 50)):
        res["family"][f"{n}x{N}"] = family(n, N)
        print(n, N, json.dumps(res["family"][f"{n}x{N}"]), flush=True)
    for n in (1024, 4096):
        for window in ((0, 0), (0, 30)):
            key = f"{n}_w{window[0]}_{window[1]}"
            res["selector"][key] = selector(n, 30, window)
            print(key, json.dumps(res["selector"][key]), flush=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
