"""Shared inputs of test_lpv_level_host.py / test_lpv_level_gpu.py: the captured reference QPs as structured
problem dicts (cmpc.structure.recognize), once per session, and the planted violations of the reference
structure (include/cmpc.h, cmpc_mpc_lpv_level)."""
import numpy as np
import scipy.sparse as sp

from conftest import lpv_qps

PER_AGENT = ("A", "B", "x0", "u_prev", "qlin", "C", "h")


def osqp_args(c):
    """(P, q, G, h, A, b) as PlannerLPV.solve hands them to osqp_solve_qp (LPV_Planner.py:156-157)."""
    Aall, l, u = c["A"], c["l"], c["u"]
    eq = np.isfinite(l) & (l == u)
    return sp.csr_matrix(c["P"]), c["q"], sp.csr_matrix(Aall[~eq]), u[~eq], sp.csr_matrix(Aall[eq]), u[eq]


_REC = {}


def recognised(name):
    """[(captured QP dict, structured single-agent dict)] of a golden file; read-only, shared between tests."""
    from cmpc import structure as St

    if name not in _REC:
        out = []
        for _, c in lpv_qps(name):
            p = St.recognize(*osqp_args(c))
            assert p is not None, name
            out.append((c, p))
        _REC[name] = out
    return _REC[name]


def stacked(name):
    """One structured batch of all captured QPs of a golden file (they share their weights); a fresh copy."""
    from cmpc import structure as St

    p = St.stack([q for _, q in recognised(name)])
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def tiled(p, batch):
    """The agents of batch dict p repeated cyclically up to `batch` agents (fresh arrays)."""
    n = p["A"].shape[0]
    idx = np.arange(batch) % n
    out = dict(p)
    for k in PER_AGENT:
        out[k] = np.ascontiguousarray(p[k][idx])
    return out


def copy_of(p):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in p.items()}


# (array, index after the stage axis, value): one violation of the pattern each
PLANTS = [
    ("A", (4, 5), 0.5),
    ("A", (6, 6), 1.0 + 2.0 ** -52),
    ("A", (8, 3), -1e-300),
    ("B", (3, 0), 0.5),
    ("B", (8, 1), 5e-324),        # the smallest denormal
    ("C", (0, 1), 1.0),
    ("C", (2, 0), 1.0),
    ("C", (4, 3), 1.0),           # a plane row: needs nb >= 1
    ("A", (0, 7), np.nan),
]


def plant(p, agent, which, k):
    """Plant violation PLANTS[which] at stage k of one agent, in place."""
    name, idx, val = PLANTS[which]
    p[name][(agent, k) + idx] = val
