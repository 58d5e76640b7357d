"""Dual solution of the structured agent QP in OSQP's form (include/cmpc.h, cmpc_mpc_duals).

With the inequalities ``G z <= h`` and the equalities ``A z = b`` of ``cmpc.structure.reference_form``
OSQP stacks ``[G; A]``, so ``y = [y_G (m) | y_A]`` and stationarity reads ``P z + q + G'y_G + A'y_A = 0``.
``y_G`` is the interior-point multiplier of the returned iterate (exactly 0 on a row whose bound is
infinite); ``y_A`` follows from ``z`` and ``y_G``:

    input-rate rows   nu_d,0 = 2 dR du_0,  nu_d,i = -2 dR du_i  (i >= 1)
    state rows        g_k = 2 Q x_k + 2 qlin_k + C_k' lambda_k  (the last term for k >= 1)
                      nu_N = -g_N,  nu_k = A_k' nu_{k+1} - g_k  (k = N-1 .. 0)
    slack rows        exactly 0

``recover`` is the numpy statement of the device kernel (csrc/mpc_dual.hip); ``recover_gpu`` runs
the kernel alone (cmpc_mpc_duals_dev) on host arrays.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib as L


def ny_of(p):
    """Length of y: m + (nx + ns)(N + 1) + nu N."""
    nx, nu, N, ns, mc = (int(p[k]) for k in ("nx", "nu", "N", "ns", "mc"))
    return N * mc + 2 * nu * N + (nx + ns) * (N + 1) + nu * N


def bounds(p):
    """(B, m) right-hand sides of G z <= h in G's row order: the stage rows, then per stage and input
    [ub_i, -lb_i]."""
    nu, N, mc = (int(p[k]) for k in ("nu", "N", "mc"))
    h = np.asarray(p["h"], float)
    B = h.shape[0]
    hu = np.stack([np.asarray(p["u_ub"], float), -np.asarray(p["u_lb"], float)], -1)   # (nu, 2)
    return np.concatenate([h.reshape(B, N * mc), np.broadcast_to(hu.ravel(), (B, N, 2 * nu)).reshape(B, -1)], 1)


def recover(p, z, lam):
    """(y, dua_res) of a structured batch ``p`` (the keys of cmpc.solver) at the primal points ``z``
    (B, nz) with the inequality multipliers ``lam`` (B, m) in G's row order.  A row of G with an
    infinite bound gets multiplier exactly 0 whatever ``lam`` holds there; an agent with a non-finite
    z gets an all-NaN y row and a NaN dua_res.  dua_res = ||P z + q + [G; A]'y||_inf."""
    nx, nu, N, ns, mc = (int(p[k]) for k in ("nx", "nu", "N", "ns", "mc"))
    ne, n, ms = nx + ns, N * nu, N * mc
    z = np.atleast_2d(np.asarray(z, float))
    lam = np.atleast_2d(np.asarray(lam, float))
    B = z.shape[0]
    cu, cd = ne * (N + 1), ne * (N + 1) + n
    Q, R, dR = (np.asarray(p[k], float).reshape(s, s) for k, s in (("Q", nx), ("R", nu), ("dR", nu)))
    Qs = np.asarray(p["Qs"], float).reshape(ns)
    A, Bm, C = (np.asarray(p[k], float) for k in ("A", "B", "C"))
    qlin = np.asarray(p["qlin"], float)
    xi = z[:, :cu].reshape(B, N + 1, ne)
    x, s = xi[..., :nx], xi[..., nx:]
    u, du = z[:, cu:cd].reshape(B, N, nu), z[:, cd:].reshape(B, N, nu)
    with np.errstate(invalid="ignore"):
        yG = np.where(np.isfinite(bounds(p)), lam.reshape(B, ms + 2 * n), 0.0)   # a select, not a product
        lk = yG[:, :ms].reshape(B, N, mc)
        lu = yG[:, ms:].reshape(B, N, nu, 2)
        drdu = 2.0 * np.einsum("jl,bil->bij", dR, du)
        nud = drdu.copy()
        nud[:, 1:] *= -1.0
        g = 2.0 * np.einsum("st,bkt->bks", Q, x) + 2.0 * qlin
        if mc:
            g[:, 1:] += np.einsum("bkrs,bkr->bks", C, lk)
        nus = np.zeros((B, N + 1, nx))
        rx = np.zeros((B, N + 1, nx))
        nus[:, N] = -g[:, N]
        for k in range(N - 1, -1, -1):
            acc = np.einsum("bjs,bj->bs", A[:, k], nus[:, k + 1])
            nus[:, k] = acc - g[:, k]
            rx[:, k] = (g[:, k] + nus[:, k]) - acc
        xiA = np.zeros((B, N + 1, ne))
        xiA[..., :nx] = nus
        y = np.concatenate([yG, xiA.reshape(B, cu), nud.reshape(B, n)], 1)
        # the u columns: 2 R u_k + y_ub - y_lb - B_k' nu_{k+1} + 2 dR du_k - 2 dR du_{k+1}
        ru = 2.0 * np.einsum("jl,bkl->bkj", R, u) + lu[..., 0] - lu[..., 1] + drdu \
            - np.einsum("bksj,bks->bkj", Bm, nus[:, 1:])
        ru[:, :-1] -= drdu[:, 1:]
        # the slack columns: 2 Qs s_k + sum over the rows on that slack of sign_r lambda_{k,r}
        rs = 2.0 * Qs * s
        sl, sg = np.asarray(p["row_slack"]), np.asarray(p["row_sign"], float)
        for r in range(mc):
            if sl[r] >= 0:
                rs[:, 1:, sl[r]] += sg[r] * lk[:, :, r]
        res = np.concatenate([np.abs(rx).reshape(B, -1), np.abs(ru).reshape(B, -1), np.abs(rs).reshape(B, -1)], 1)
        dua = res.max(1) if res.shape[1] else np.zeros(B)
    bad = ~np.isfinite(z).all(1)
    y[bad] = np.nan
    dua = np.where(bad, np.nan, dua)
    return y, dua


def recover_gpu(p, z, lam, ctx=None):
    """``recover`` by the device kernel alone (cmpc_mpc_duals_dev): host arrays in, (y, dua_res) out."""
    import torch

    from .solver import _dims, _tptr, _weights

    ctx = ctx or L.default_context()
    z = np.atleast_2d(L.f64(z))
    B = z.shape[0]
    dev = torch.device("cuda", ctx.device)
    up = {k: torch.from_numpy(L.f64(p[k])).to(dev) for k in ("A", "B", "qlin", "C", "h")}
    zt = torch.from_numpy(z).to(dev)
    lt = torch.from_numpy(np.atleast_2d(L.f64(lam))).to(dev)
    y = torch.empty((B, ny_of(p)), dtype=torch.float64, device=dev)
    dr = torch.empty(B, dtype=torch.float64, device=dev)
    w, keep = _weights(p)
    data = L.cmpc_mpc_data(_tptr(up["A"]), _tptr(up["B"]), None, None, _tptr(up["qlin"]), _tptr(up["C"]),
                           _tptr(up["h"]))
    du = L.cmpc_mpc_duals(_tptr(y), _tptr(dr))
    s = torch.cuda.current_stream(dev)
    ctx.check(ctx.lib.cmpc_mpc_duals_dev(ctx.h, ct.byref(_dims(p, B)), ct.byref(w), ct.byref(data), _tptr(zt),
                                         _tptr(lt), ct.byref(du), ct.c_void_p(s.cuda_stream)))
    s.synchronize()
    del keep
    return y.cpu().numpy(), dr.cpu().numpy()
