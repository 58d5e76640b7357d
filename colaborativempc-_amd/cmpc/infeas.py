"""Primal-infeasibility certificate of the structured agent QP (include/cmpc.h, cmpc_mpc_cert): OSQP's status -3
with its ``res.prim_inf_cert``, by single-row reachability.

A hard stage row (k, r) — ``row_slack[r] == -1``, finite ``h[k, r]`` — asks ``c'x_k <= h`` with ``c = C[k, r]``.
The adjoint recursion

    p_k = c,   g_j = B_j' p_{j+1},   p_j = A_j' p_{j+1}     (j = k-1 .. 0)

gives ``c'x_k = p_0'x0 + sum_j g_j'u_j``, so over the input box the row's smallest value is

    reach = p_0'x0 + sum_{j<k, i} min(g_ji lb_i, g_ji ub_i)

(a term with ``g_ji == 0`` counts 0; a term whose minimising bound is infinite disqualifies the row), and with
``S = |h| + sum_s |p_0s x0_s| + sum_{j,i} |g_ji| |that bound|`` the QP is infeasible when
``reach - h > CMPC_CERT_TOL * S``.  The winner among an agent's candidates is the largest ``(reach - h) / S``, ties
to the smallest k, then r; a candidate whose ratio is not finite is no candidate.  The Farkas ray, in the layout
of ``cmpc.duals`` (``[y_G | y_A]``, OSQP order): 1 at row (k, r); ``t = -g_ji`` on the ``u_i <= ub_i`` row when
``t > 0``, ``-t`` on the ``-u_i <= -lb_i`` row when ``t < 0``; ``nu_j = -p_j`` on the state rows ``j <= k``; 0
elsewhere.  Then ``G'y_G + A'y_A = 0`` and ``h'y_G + b'y_A = -(reach - h) < 0``.

The certificate is sufficient, not necessary: infeasibility that needs two or more rows combined gets none from
this rule; ``certify_rows`` below (csrc/mpc_infeas_rows.hip) covers hard rows that contradict each other.

``certify`` is the numpy statement of the device kernel (csrc/mpc_infeas.hip); ``certify_gpu`` runs the kernel
alone (cmpc_mpc_certify) on host arrays; ``verify`` checks a ray against any reference-form matrices.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib as L
from .duals import ny_of

CERT_TOL = L.CMPC_CERT_TOL


def _examined(status, B):
    if status is None:
        return np.ones(B, bool)
    st = np.asarray(status).reshape(B)
    return ~((st == L.CMPC_SOLVED) | (st == L.CMPC_SOLVED_INACCURATE))


def certify(p, status=None):
    """The certificate of every agent of the structured batch ``p`` (the keys of cmpc.solver) whose ``status``
    (B,) is not 1 or 2 (None: every agent).  Returns dict(row (B,) int32: (k-1) mc + r when certified, else -1;
    margin (B,): the best candidate's (reach - h) / S, NaN without a candidate; ray (B, ny): the Farkas ray when
    certified, else NaN; status (B,) int32: ``status`` (zeros when None) with -3 at the certified agents).  An
    agent that is not examined keeps row -1, NaN margin and a NaN ray."""
    nx, nu, N, ns, mc = (int(p[k]) for k in ("nx", "nu", "N", "ns", "mc"))
    ne, ms = nx + ns, N * mc
    m = ms + 2 * nu * N
    A, Bm, C, h, x0 = (np.asarray(p[k], float) for k in ("A", "B", "C", "h", "x0"))
    B = A.shape[0]
    lb, ub = np.asarray(p["u_lb"], float).reshape(nu), np.asarray(p["u_ub"], float).reshape(nu)
    hard = np.nonzero(np.asarray(p["row_slack"]).reshape(mc) < 0)[0]
    row = -np.ones(B, np.int32)
    margin = np.full(B, np.nan)
    ray = np.full((B, ny_of(p)), np.nan)
    st = np.zeros(B, np.int32) if status is None else np.array(status, np.int32).reshape(B)
    if (lb > ub).any() or hard.size == 0:
        return dict(row=row, margin=margin, ray=ray, status=st)
    ks = np.repeat(np.arange(N), hard.size)       # candidate q = (k-1) nh + index: stage k = ks + 1
    rs = np.tile(hard, N)
    for b in np.nonzero(_examined(status, B))[0]:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            P = C[b, ks, rs].copy()                                   # (ncand, nx)
            hv = h[b, ks, rs]
            reach, S = np.zeros(ks.size), np.zeros(ks.size)
            disq = np.zeros(ks.size, bool)
            for j in range(N - 1, -1, -1):
                on = j <= ks
                g = P @ Bm[b, j]                                      # (ncand, nu): B_j' p
                bnd = np.where(g > 0.0, lb, ub)
                term = on[:, None] & (g != 0.0)
                fin = np.isfinite(bnd)
                disq |= (term & ~fin).any(1)
                use = term & fin
                gz, bz = np.where(use, g, 0.0), np.where(use, bnd, 0.0)
                reach += (gz * bz).sum(1)
                S += (np.abs(gz) * np.abs(bz)).sum(1)
                P = np.where(on[:, None], P @ A[b, j], P)             # A_j' p
            v = P * x0[b]
            reach += v.sum(1)
            S += np.abs(v).sum(1) + np.abs(hv)
            d = reach - hv
            ratio = d / S
            valid = ~disq & np.isfinite(hv) & np.isfinite(ratio)
        if not valid.any():
            continue
        q = int(np.argmax(np.where(valid, ratio, -np.inf)))          # the first maximum: smallest k, then r
        margin[b] = ratio[q]
        if not d[q] > CERT_TOL * S[q]:
            continue
        k, r = int(ks[q]) + 1, int(rs[q])
        row[b] = (k - 1) * mc + r
        st[b] = L.CMPC_PRIMAL_INFEASIBLE
        y = np.zeros(ray.shape[1])
        y[row[b]] = 1.0
        pj = C[b, k - 1, r].copy()
        for j in range(k - 1, -1, -1):
            y[m + (j + 1) * ne: m + (j + 1) * ne + nx] = -pj
            t = -(pj @ Bm[b, j])
            y[ms + 2 * j * nu: ms + 2 * (j + 1) * nu: 2] = np.where(t > 0.0, t, 0.0)
            y[ms + 2 * j * nu + 1: ms + 2 * (j + 1) * nu: 2] = np.where(t < 0.0, -t, 0.0)
            pj = pj @ A[b, j]
        y[m: m + nx] = -pj
        ray[b] = y
    return dict(row=row, margin=margin, ray=ray, status=st)


def verify(G, h, A, b, y):
    """(||[G; A]'y||_inf, h'y_G + b'y_A) of a candidate ray ``y`` (OSQP order [G rows; A rows]) on any
    reference-form matrices (dense or scipy sparse).  A row of G with an infinite bound is inactive: its entry of
    y counts as 0 in both figures (the select of cmpc.duals).  A Farkas ray has a zero first figure, a negative
    second and y_G >= 0."""
    h = np.asarray(h, float).ravel()
    b = np.asarray(b, float).ravel()
    y = np.asarray(y, float).ravel()
    mi = h.size
    fin = np.isfinite(h)
    yG = np.where(fin, y[:mi], 0.0)
    yA = y[mi:]
    r = np.asarray(G.T @ yG).ravel() + np.asarray(A.T @ yA).ravel()
    gap = float(np.where(fin, h, 0.0) @ yG + b @ yA)
    return float(np.abs(r).max(initial=0.0)), gap


def certify_dev(shared, dev, status=None, ray=None, margin=None, row=None, ctx=None, stream=None):
    """The certificate launch on device-resident data (cmpc_mpc_certify_dev; one launch on ``stream``, default
    torch's current one, no host synchronisation).  ``shared``: dims + shared weights (host); ``dev``: CUDA float64
    tensors A, B, x0, C, h; ``status`` (B,) int32, in-out, None: every agent examined; ``ray`` (B, ny) / ``margin``
    (B,) float64 and ``row`` (B,) int32: optional outputs (one of ``status`` and these is needed)."""
    import torch

    from .solver import _dims, _tptr, _weights

    ctx = ctx or L.default_context(dev["A"].device.index or 0)
    w, keep = _weights(shared)
    data = L.cmpc_mpc_data(_tptr(dev["A"]), _tptr(dev["B"]), _tptr(dev["x0"]), None, None, _tptr(dev["C"]),
                           _tptr(dev["h"]))
    cert = L.cmpc_mpc_cert(_tptr(ray), _tptr(margin), _tptr(row))
    s = stream if stream is not None else torch.cuda.current_stream(dev["A"].device)
    ctx.check(ctx.lib.cmpc_mpc_certify_dev(ctx.h, ct.byref(_dims(shared, int(dev["A"].shape[0]))), ct.byref(w),
                                           ct.byref(data), _tptr(status), ct.byref(cert),
                                           ct.c_void_p(s.cuda_stream)))
    del keep


def certify_gpu(p, status=None, ctx=None):
    """``certify`` by the device kernel alone (cmpc_mpc_certify): host arrays in, the same dict out."""
    from .solver import _dims, _weights, check_shapes

    ctx = ctx or L.default_context()
    B = int(np.shape(p["A"])[0])
    check_shapes(p, B)
    w, keep = _weights(p)
    arrs = {k: L.f64(p[k]) for k in ("A", "B", "x0", "C", "h")}
    data = L.cmpc_mpc_data(L.dptr(arrs["A"]), L.dptr(arrs["B"]), L.dptr(arrs["x0"]), None, None, L.dptr(arrs["C"]),
                           L.dptr(arrs["h"]))
    row = -np.ones(B, np.int32)
    margin = np.full(B, np.nan)
    ray = np.full((B, ny_of(p)), np.nan)
    st = None if status is None else np.array(status, np.int32).reshape(B)
    cert = L.cmpc_mpc_cert(L.dptr(ray), L.dptr(margin), L.iptr(row))
    ctx.check(ctx.lib.cmpc_mpc_certify(ctx.h, ct.byref(_dims(p, B)), ct.byref(w), ct.byref(data), L.iptr(st),
                                       ct.byref(cert)))
    del keep, arrs
    if st is None:   # a NULL status: every agent examined
        st = np.where(row >= 0, L.CMPC_PRIMAL_INFEASIBLE, 0).astype(np.int32)
    return dict(row=row, margin=margin, ray=ray, status=st)


# ---- infeasibility that needs several hard rows combined (csrc/mpc_infeas_rows.hip) ----
#
# The hard rows H (row_slack == -1, finite h), the dynamics and the input box are infeasible together exactly when
# the least-squares violation  min over the box of 1/2 ||(C x(u) - h)_+||^2  is positive, and at its minimiser the
# violation vector is a Farkas ray.  Accelerated projected gradient (FISTA: no restart, no line search) proposes
# the violation vector v >= 0 of its iterate as row weights; the aggregated row  sum_H w_kr C_kr x_k <= w'h  with
# w = v / max v then takes the single-row reachability test, which alone decides.  The certificate is sufficient
# and is for infeasibility by a margin: the iterations needed grow roughly as 1 / gap.
CERT_ROWS_MAX_ITER = L.CMPC_CERT_ROWS_MAX_ITER
CERT_ROWS_CHECK_EVERY = L.CMPC_CERT_ROWS_CHECK_EVERY


def _examined_rows(status, B):
    if status is None:
        return np.ones(B, bool)
    st = np.asarray(status).reshape(B)
    return ~((st == L.CMPC_SOLVED) | (st == L.CMPC_SOLVED_INACCURATE) | (st == L.CMPC_PRIMAL_INFEASIBLE))


def _clip(v, lb, ub):
    """lb where v < lb, ub where the result > ub: a NaN bound never clips, a NaN v stays."""
    v = np.where(v < lb, lb, v)
    return np.where(v > ub, ub, v)


def certify_rows(p, status=None, max_iter=CERT_ROWS_MAX_ITER, check_every=CERT_ROWS_CHECK_EVERY):
    """The combined-row certificate of every agent of the structured batch ``p`` whose ``status`` (B,) is not 1, 2
    or -3 (None: every agent): the numpy statement of csrc/mpc_infeas_rows.hip.

    Per agent, with H the hard stage rows of finite h (none, or ``u_lb_i > u_ub_i`` for an input: no candidate):
      Lf    = sum over H of sum_{j<k, i} g_ji^2, g the row's adjoint coefficients (``certify``); not finite or not
              > 0: no candidate
      u     = clip(0, lb, ub), y = u, t = 1; then for it = 1 .. max_iter:
                x forward from x0 with inputs y; v = max(C x - h, 0) on H (a NaN stays)
                backwards  P <- P + sum_{r: v_kr != 0} C_kr v_kr,  g_j = B_j' P,  P <- A_j' P
                u+ = clip(y - g (1 / Lf), lb, ub);  t+ = (1 + sqrt(1 + 4 t^2)) / 2;  y = u+ + ((t - 1) / t+)(u+ - u)
      check   when it % check_every == 0 and at it == max_iter: w = max(C x(u) - h, 0) on H at u (not y).
              max w not > 0: stop without a certificate (margin 0 when every hard row holds at u, NaN on NaN data).
              Else w <- w / max w, the aggregated adjoint  P_N = C_N' w_N, P_j = C_j' w_j + A_j' P_{j+1},
              P_0 = A_0' P_1, g_j = B_j' P_{j+1}, and
                reach = P_0'x0 + sum min(g_ji lb_i, g_ji ub_i)   (g_ji == 0 counts 0; an infinite minimising bound
                                                                  disqualifies: NaN margin)
                S     = sum |w h| + sum_s |P_0s x0_s| + sum |g_ji| |that bound|,   d = reach - w'h
              certified, and stopped, when d > CMPC_CERT_TOL * S.

    Returns dict(status (B,) int32: ``status`` (zeros when None) with -3 at the certified agents; ray (B, ny), the
    cmpc.duals layout: w on the stage rows, ``t = -g_ji`` split by sign onto input i's two box rows of stage j,
    ``nu_j = -P_j`` on the state rows, 0 on slack and input-rate rows; all NaN for an examined agent without a
    certificate; margin (B,): d / S of the last check, NaN without one; iters (B,) int32: iterations done; nrows (B,)
    int32: rows with w != 0 at the last check; scale (B,): that check's S (not a device output)).  An agent that is
    not examined keeps NaN / 0 everywhere."""
    nx, nu, N, ns, mc = (int(p[k]) for k in ("nx", "nu", "N", "ns", "mc"))
    ne, ms = nx + ns, N * mc
    m = ms + 2 * nu * N
    A, Bm, C, h, x0 = (np.asarray(p[k], float) for k in ("A", "B", "C", "h", "x0"))
    B = A.shape[0]
    lb, ub = np.asarray(p["u_lb"], float).reshape(nu), np.asarray(p["u_ub"], float).reshape(nu)
    hard = np.asarray(p["row_slack"]).reshape(mc) < 0
    max_iter = int(max_iter) if max_iter and max_iter > 0 else CERT_ROWS_MAX_ITER
    check_every = int(check_every) if check_every and check_every > 0 else CERT_ROWS_CHECK_EVERY
    margin, scale = np.full(B, np.nan), np.full(B, np.nan)
    ray = np.full((B, ny_of(p)), np.nan)
    iters, nrows = np.zeros(B, np.int32), np.zeros(B, np.int32)
    st = np.zeros(B, np.int32) if status is None else np.array(status, np.int32).reshape(B)
    out = dict(status=st, ray=ray, margin=margin, iters=iters, nrows=nrows, scale=scale)
    if (lb > ub).any() or not hard.any():
        return out
    for b in np.nonzero(_examined_rows(status, B))[0]:
        Ab, Bb, Cb, hb, xb = A[b], Bm[b], C[b], h[b], x0[b]
        Hm = hard[None, :] & np.isfinite(hb)                               # (N, mc)
        if not Hm.any():
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            # ---- Lf: every row's adjoint coefficients (the recursion of ``certify``, all rows at once)
            ks, rs = np.nonzero(Hm)
            P = Cb[ks, rs].copy()
            Lf = 0.0
            for j in range(N - 1, -1, -1):
                on = j <= ks
                g = P @ Bb[j]
                Lf += float((np.where(on[:, None], g, 0.0) ** 2).sum())
                P = np.where(on[:, None], P @ Ab[j], P)
            if not (np.isfinite(Lf) and Lf > 0.0):
                continue
            step = 1.0 / Lf

            def forward(uu):
                x, V = xb, np.zeros((N, mc))
                for j in range(N):
                    x = Ab[j] @ x + Bb[j] @ uu[j]
                    cv = Cb[j] @ x - hb[j]
                    V[j] = np.where(Hm[j] & ((cv > 0.0) | (cv != cv)), cv, 0.0)
                return V

            def backward(V):
                """(g (N, nu), P_j (N + 1, nx)) of the weights V"""
                P, G, Ps = np.zeros(nx), np.zeros((N, nu)), np.zeros((N + 1, nx))
                for j in range(N - 1, -1, -1):
                    nz = V[j] != 0.0
                    if nz.any():
                        P = P + V[j][nz] @ Cb[j][nz]
                    Ps[j + 1] = P
                    G[j] = P @ Bb[j]
                    P = P @ Ab[j]
                Ps[0] = P
                return G, Ps

            u = _clip(np.zeros((N, nu)), lb, ub)
            y, t = u.copy(), 1.0
            cert = False
            for it in range(1, max_iter + 1):
                G, _ = backward(forward(y))
                un = _clip(y - G * step, lb, ub)
                tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
                y = un + ((t - 1.0) / tn) * (un - u)
                u, t = un, tn
                iters[b] = it
                if it % check_every and it != max_iter:
                    continue
                w = forward(u)
                mw = np.where(np.isnan(w).any(), np.nan, w.max())
                if not mw > 0.0:
                    margin[b], scale[b], nrows[b] = (0.0 if mw == 0.0 else np.nan), np.nan, 0
                    break
                w = w / mw
                G, Ps = backward(w)
                bnd = np.where(G > 0.0, lb, ub)
                term = G != 0.0
                fin = np.isfinite(bnd)
                disq = bool((term & ~fin).any())
                use = term & fin
                gz, bz = np.where(use, G, 0.0), np.where(use, bnd, 0.0)
                px = Ps[0] * xb
                nzw = w != 0.0
                wh = w[nzw] * hb[nzw]
                reach = px.sum() + (gz * bz).sum()
                S = np.abs(wh).sum() + np.abs(px).sum() + (np.abs(gz) * np.abs(bz)).sum()
                d = reach - wh.sum()
                nrows[b] = int(nzw.sum())
                margin[b], scale[b] = (np.nan, np.nan) if disq else (d / S, S)
                if not disq and d > CERT_TOL * S:
                    cert = True
                    break
        if not cert:
            continue
        st[b] = L.CMPC_PRIMAL_INFEASIBLE
        yr = np.zeros(ray.shape[1])
        yr[:ms] = w.ravel()
        tt = -G
        yr[ms:m:2] = np.where(tt > 0.0, tt, 0.0).ravel()
        yr[ms + 1:m:2] = np.where(tt < 0.0, -tt, 0.0).ravel()
        for j in range(N + 1):
            yr[m + j * ne: m + j * ne + nx] = -Ps[j]
        ray[b] = yr
    return out


def certify_rows_dev(shared, dev, status=None, ray=None, margin=None, iters=None, nrows=None, max_iter=0,
                     check_every=0, ctx=None, stream=None):
    """The combined-row certificate launch on device-resident data (cmpc_mpc_certify_rows_dev; one launch on
    ``stream``, default torch's current one, no host synchronisation).  Arguments as ``certify_dev``; ``iters`` and
    ``nrows`` (B,) int32 optional outputs; ``max_iter`` / ``check_every`` <= 0: the library's defaults."""
    import torch

    from .solver import _dims, _tptr, _weights

    ctx = ctx or L.default_context(dev["A"].device.index or 0)
    w, keep = _weights(shared)
    data = L.cmpc_mpc_data(_tptr(dev["A"]), _tptr(dev["B"]), _tptr(dev["x0"]), None, None, _tptr(dev["C"]),
                           _tptr(dev["h"]))
    cert = L.cmpc_mpc_cert_rows(_tptr(ray), _tptr(margin), _tptr(iters), _tptr(nrows))
    s = stream if stream is not None else torch.cuda.current_stream(dev["A"].device)
    ctx.check(ctx.lib.cmpc_mpc_certify_rows_dev(ctx.h, ct.byref(_dims(shared, int(dev["A"].shape[0]))), ct.byref(w),
                                                ct.byref(data), _tptr(status), ct.byref(cert), int(max_iter),
                                                int(check_every), ct.c_void_p(s.cuda_stream)))
    del keep


def certify_rows_gpu(p, status=None, max_iter=0, check_every=0, ctx=None):
    """``certify_rows`` by the device kernel alone (cmpc_mpc_certify_rows): host arrays in, the same dict out
    (without ``scale``)."""
    from .solver import _dims, _weights, check_shapes

    ctx = ctx or L.default_context()
    B = int(np.shape(p["A"])[0])
    check_shapes(p, B)
    w, keep = _weights(p)
    arrs = {k: L.f64(p[k]) for k in ("A", "B", "x0", "C", "h")}
    data = L.cmpc_mpc_data(L.dptr(arrs["A"]), L.dptr(arrs["B"]), L.dptr(arrs["x0"]), None, None, L.dptr(arrs["C"]),
                           L.dptr(arrs["h"]))
    margin = np.full(B, np.nan)
    ray = np.full((B, ny_of(p)), np.nan)
    iters, nrows = np.zeros(B, np.int32), np.zeros(B, np.int32)
    st = np.zeros(B, np.int32) if status is None else np.array(status, np.int32).reshape(B)
    cert = L.cmpc_mpc_cert_rows(L.dptr(ray), L.dptr(margin), L.iptr(iters), L.iptr(nrows))
    ctx.check(ctx.lib.cmpc_mpc_certify_rows(ctx.h, ct.byref(_dims(p, B)), ct.byref(w), ct.byref(data), L.iptr(st),
                                            ct.byref(cert), int(max_iter), int(check_every)))
    del keep, arrs
    return dict(status=st, ray=ray, margin=margin, iters=iters, nrows=nrows)
