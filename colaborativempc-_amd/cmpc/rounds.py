"""Device-resident consensus-round driver (the collaborative loop of
planner/scripts/LPV_HP_N_main.py:96-120, and of the one-process-per-agent ROS
variant ROS/src/planner_experiments/src/LPV_ROS_main.py:124-150, re-designed as
one process per GPU).

Each round, on the GPU and on one stream:
  0. select  — optional (`reselect=r`, every r rounds): each local agent's nb nearest
               other agents from the exchanged trajectories, into the neighbour
               table in place                              (cmpc_nbr_select_dev)
  1. build   — every local agent's stage rows / linear cost from the previous
               round's exchanged trajectories            (cmpc_di_build_dev)
  2. solve   — batched condensed IPM, one wavefront per agent  (cmpc_solve_mpc_batch_dev)
  3. advance — x0 <- x_1, u_prev <- u_0, local trajectory <- predicted positions
               (LPV_HP_N_main.py:106-117)                (cmpc_di_advance_dev)
     (fused: 1-3 are one launch, cmpc_di_round_dev)
  4. exchange — all-gather of the (N+1) x 2 fp64 predicted positions of every
               agent over RCCL (torch.distributed "nccl" backend) — the
               replacement of the ROS topic exchange / np.swapaxes at :117.

Agents are sharded contiguously across ranks (they are ordered along the road,
so most neighbours are local); every rank holds the full gathered trajectory
buffer, which is what a Jacobi round needs.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib as L
from .solver import _dims, _tptr, _weights, nz_of


def exchange_positions(traj_all, traj_local, world=1, group=None, comm=None):
    """The per-round exchange of predicted positions (the np.swapaxes "exchange" of
    LPV_HP_N_main.py:117, and the ROS topic publish/subscribe of LPV_ROS_main.py:66-77):
    every rank's contiguous block `traj_local` (B, N+1, 2) is gathered, in rank order,
    into the node-global `traj_all` (world*B, N+1, 2).  One all-gather per round;
    over RCCL/xGMI with the "nccl" backend, gloo on CPU tensors."""
    if comm is not None:   # libcmpc's own RCCL communicator (cmpc.comm.Comm), no torch.distributed
        comm.allgather(traj_local, traj_all)
        return
    if world == 1:
        traj_all.copy_(traj_local)
        return
    import torch.distributed as dist

    if traj_all.shape[0] != world * traj_local.shape[0]:
        raise ValueError("traj_all must hold world x local agents")
    if traj_all.is_cuda and dist.get_backend(group) == "gloo":
        # gloo moves host memory only: stage through the host (multi-process runs sharing one
        # GPU, or hosts without RCCL); the gathered rows are the same bytes in the same order
        host = traj_all.new_empty(traj_all.shape, device="cpu")
        dist.all_gather_into_tensor(host, traj_local.detach().cpu().contiguous(), group=group)
        traj_all.copy_(host)
        return
    dist.all_gather_into_tensor(traj_all, traj_local.contiguous(), group=group)


def select_neighbours_dev(traj_all, nb, batch=None, self_offset=0, window=(0, 0), out=None, dist2=None, ctx=None,
                          stream=None):
    """The ``nb`` nearest other agents of the local agents [self_offset, self_offset + batch) (default: all)
    out of the exchange buffer ``traj_all`` (n_total, N+1, 2), a contiguous fp64 CUDA tensor — one launch of
    cmpc_nbr_select_dev on ``stream`` (default: torch's current one), no host synchronisation.  The rule is
    ``scenarios.select_neighbours``'s (score = min over the stages of ``window`` of the squared distance, ties
    by index, the agent itself left out by index), the result bit-equal to it.  Writes the (batch, nb) int32
    global indices, nearest first, into ``out`` (allocated when None) and returns it; ``dist2`` (batch, nb)
    fp64, optional, receives their scores.  Nearest first is not the reference's index order of ns[i]: it
    only reorders an agent's collision rows and the columns of ``planes``.  A buffer (n_total, N+1, 3) is scored
    by the 3-D distance (cmpc_nbr_select3_dev)."""
    import torch

    if traj_all.dim() != 3 or traj_all.shape[2] not in (2, 3) or traj_all.dtype != torch.float64 or \
            not traj_all.is_cuda or not traj_all.is_contiguous():
        raise ValueError("traj_all: a contiguous (n_total, N+1, 2) or (n_total, N+1, 3) float64 CUDA tensor")
    n_total, N = int(traj_all.shape[0]), int(traj_all.shape[1]) - 1
    batch = n_total - self_offset if batch is None else int(batch)
    if out is None:
        out = torch.empty((max(batch, 0), max(int(nb), 0)), dtype=torch.int32, device=traj_all.device)
    for name, t, dt in (("out", out, torch.int32), ("dist2", dist2, torch.float64)):
        if t is not None and (t.device != traj_all.device or t.dtype != dt or tuple(t.shape) != (batch, nb) or
                              not t.is_contiguous()):
            raise ValueError(f"{name}: need a contiguous ({batch}, {nb}) {dt} tensor on {traj_all.device}")
    ctx = ctx or L.default_context(traj_all.device.index)
    if stream is None:
        stream = torch.cuda.current_stream(traj_all.device)
    dims = L.cmpc_nbr_dims(batch, N, int(nb), int(self_offset), n_total, int(window[0]), int(window[1]))
    select = ctx.lib.cmpc_nbr_select3_dev if traj_all.shape[2] == 3 else ctx.lib.cmpc_nbr_select_dev
    ctx.check(select(ctx.h, ct.byref(dims), _tptr(traj_all), _tptr(out), None if dist2 is None else _tptr(dist2),
                     ct.c_void_p(getattr(stream, "cuda_stream", stream))))
    return out


def order_by_iters_dev(iters, out=None, ctx=None, stream=None):
    """The longest-first launch order of ``cmpc_opts.order`` from a round's per-agent IPM iteration counts
    ``iters`` (batch,), a contiguous int32 CUDA tensor — one launch of cmpc_order_by_iters_dev on ``stream``
    (default: torch's current one), no host synchronisation.  The rule is ``scenarios.order_by_iters``'s
    (descending min(max(iters, 0), 65535), equal keys in index order), the result equal to it and always a
    permutation.  Writes the (batch,) int32 order into ``out`` (allocated when None; it must not alias
    ``iters``) and returns it."""
    import torch

    if not isinstance(iters, torch.Tensor) or iters.dim() != 1 or iters.dtype != torch.int32 or not iters.is_cuda or \
            not iters.is_contiguous():
        raise ValueError("iters: a contiguous (batch,) int32 CUDA tensor")
    batch = int(iters.shape[0])
    if out is None:
        out = torch.empty(batch, dtype=torch.int32, device=iters.device)
    if not isinstance(out, torch.Tensor) or out.device != iters.device or out.dtype != torch.int32 or \
            tuple(out.shape) != (batch,) or not out.is_contiguous():
        raise ValueError(f"out: need a contiguous ({batch},) torch.int32 tensor on {iters.device}")
    ctx = ctx or L.default_context(iters.device.index)
    if stream is None:
        stream = torch.cuda.current_stream(iters.device)
    ctx.check(ctx.lib.cmpc_order_by_iters_dev(ctx.h, batch, _tptr(iters), _tptr(out),
                                              ct.c_void_p(getattr(stream, "cuda_stream", stream))))
    return out


def log_round_dev(z, nx, nu, ns, N, look_col, row=None, kkt=None, iters=None, status=None, ctx=None, stream=None):
    """A round's log rows on the device — one launch of cmpc_round_log_dev on ``stream`` (default: torch's current
    one), no host synchronisation: out of the round's ``z`` (batch, nz), a contiguous fp64 CUDA tensor in the
    reference layout, ``row["state"]`` (batch, nx) <- xPred[0], ``row["u"]`` (batch, nu) <- uPred[0],
    ``row["look_ahead"]`` (batch,) <- xPred[-1, look_col] - xPred[0, look_col], and ``row["kkt" | "iters" |
    "status"]`` (batch,) <- the solver outputs ``kkt`` / ``iters`` / ``status`` of the round — the rule of
    ``scenarios.log_row``, bit for bit.  ``row``: dict of destination tensors, e.g. one row per round of a
    preallocated history; a key that is missing or None is skipped.  None: state, u and look_ahead are
    allocated, and kkt / iters / status where the source is given.  Returns ``row``.  What the round handles do
    with ``log=``; the torch-driven ``LPVRounds`` / ``DIRounds`` hold their tensors and call this."""
    import torch

    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype != torch.float64 or not z.is_cuda or \
            not z.is_contiguous():
        raise ValueError("z: a contiguous (batch, nz) float64 CUDA tensor")
    batch = int(z.shape[0])
    if z.shape[1] != (nx + ns) * (N + 1) + 2 * nu * N:
        raise ValueError("z: nz = (nx+ns)(N+1) + 2 nu N")
    shapes = dict(state=((batch, nx), torch.float64), u=((batch, nu), torch.float64),
                  look_ahead=((batch,), torch.float64), kkt=((batch,), torch.float64),
                  iters=((batch,), torch.int32), status=((batch,), torch.int32))
    src = dict(kkt=kkt, iters=iters, status=status)
    if row is None:
        row = {k: torch.empty(shp, dtype=dt, device=z.device) for k, (shp, dt) in shapes.items()
               if k not in src or src[k] is not None}
    for k, t in list(row.items()) + list(src.items()):
        if k not in shapes:
            raise ValueError(f"row: unknown destination {k!r}")
        shp, dt = shapes[k]
        if t is not None and (not isinstance(t, torch.Tensor) or t.device != z.device or t.dtype != dt or
                              tuple(t.shape) != shp or not t.is_contiguous()):
            raise ValueError(f"{k}: need a contiguous {shp} {dt} tensor on {z.device}")
    if batch == 0:   # empty tensors have no address to hand over; the entry point launches nothing either
        return row
    ctx = ctx or L.default_context(z.device.index)
    if stream is None:
        stream = torch.cuda.current_stream(z.device)
    dims = L.cmpc_log_dims(batch, int(nx), int(nu), int(ns), int(N), int(look_col))
    dst = L.cmpc_log_row(*[_tptr(row.get(k)) for k in ("state", "u", "look_ahead", "kkt", "iters", "status")])
    ctx.check(ctx.lib.cmpc_round_log_dev(ctx.h, ct.byref(dims), _tptr(z), _tptr(kkt), _tptr(iters), _tptr(status),
                                         ct.byref(dst), ct.c_void_p(getattr(stream, "cuda_stream", stream))))
    return row


def _lin_params(prm):
    """cmpc_lin_params of a ``prm`` dict(ix, iy, min_dist, wq); cmpc_lin3_params when it has ``iz``."""
    if "iz" in prm:
        return L.cmpc_lin3_params(int(prm["ix"]), int(prm["iy"]), int(prm["iz"]), float(prm["min_dist"]),
                                  float(prm["wq"]))
    return L.cmpc_lin_params(int(prm["ix"]), int(prm["iy"]), float(prm["min_dist"]), float(prm["wq"]))


def _pos_dim(prm):
    """Coordinates of a position under ``prm``: 3 with ``iz`` (the cmpc_lin3_* entries, buffers x 3), else 2."""
    return 3 if "iz" in prm else 2


def _lin_fn(ctx, prm, name):
    """The family's device entry ``name`` ("build_dev", ..) for ``prm``: cmpc_lin3_<name> with ``iz``, else
    cmpc_lin_<name>."""
    return getattr(ctx.lib, ("cmpc_lin3_" if "iz" in prm else "cmpc_lin_") + name)


def _lin_args(traj_all, nbr, own, self_offset, ctx, stream, pd=2):
    """What the three linear-model wrappers share: the shapes read off the tensors, cmpc_lin_dims, cmpc_lin_own."""
    import torch

    q = own["qlin_own"]
    B, N, nx = int(q.shape[0]), int(q.shape[1]) - 1, int(q.shape[2])
    C_own, h_own = own.get("C_own"), own.get("h_own")
    mo = 0 if C_own is None else int(C_own.shape[2])
    nb = 0 if nbr is None else int(nbr.shape[1])
    if traj_all.dim() != 3 or tuple(traj_all.shape[1:]) != (N + 1, pd) or (mo and tuple(h_own.shape) != (B, N, mo)):
        raise ValueError(f"traj_all (n_total, N+1, {pd}), qlin_own (B, N+1, nx), C_own (B, N, mo, nx), h_own (B, N, mo)")
    ctx = ctx or L.default_context(traj_all.device.index)
    if stream is None:
        stream = torch.cuda.current_stream(traj_all.device)
    dims = L.cmpc_lin_dims(B, N, nb, int(self_offset), nx, mo)
    lo = L.cmpc_lin_own(_tptr(q), _tptr(C_own) if mo else None, _tptr(h_own) if mo else None)
    return ctx, dims, lo, (_tptr(nbr) if nb and B else None), ct.c_void_p(getattr(stream, "cuda_stream", stream))


def lin_build_dev(prm, own, nbr, traj_all, self_offset=0, out=None, ctx=None, stream=None):
    """The linear-model family's builder on the device — one launch of cmpc_lin_build_dev on ``stream`` (default:
    torch's current one), no host synchronisation; the rule is ``scenarios.lin_rows``'s, bit for bit.  ``prm``:
    dict(ix, iy, min_dist, wq); ``own``: dict of contiguous fp64 CUDA tensors qlin_own (B, N+1, nx), C_own
    (B, N, mo, nx), h_own (B, N, mo) (the last two None when mo = 0); ``nbr`` (B, nb) int32 (None when nb = 0);
    ``traj_all`` (n_total, N+1, 2).  Writes ``out`` = (qlin, C, h) (allocated when None) and returns it."""
    import torch

    ctx, dims, lo, pn, st = _lin_args(traj_all, nbr, own, self_offset, ctx, stream, _pos_dim(prm))
    B, N, nx, mc = dims.batch, dims.N, dims.nx, dims.mo + dims.nb
    if out is None:
        out = tuple(torch.empty(shp, dtype=torch.float64, device=traj_all.device)
                    for shp in ((B, N + 1, nx), (B, N, mc, nx), (B, N, mc)))
    qlin, C, h = out
    if (tuple(qlin.shape), tuple(C.shape), tuple(h.shape)) != ((B, N + 1, nx), (B, N, mc, nx), (B, N, mc)):
        raise ValueError("out: qlin (B, N+1, nx), C (B, N, mo+nb, nx), h (B, N, mo+nb)")
    if B == 0 or mc == 0:   # empty tensors have no address to hand over; nothing to build beyond the copy of qlin
        qlin.copy_(own["qlin_own"])
        return out
    ctx.check(_lin_fn(ctx, prm, "build_dev")(ctx.h, ct.byref(_lin_params(prm)), ct.byref(dims), pn, ct.byref(lo),
                                             _tptr(traj_all), _tptr(qlin), _tptr(C), _tptr(h), st))
    return out


def lin_advance_dev(prm, z, nx, nu, ns, N, x0, u_prev, traj_local, ctx=None, stream=None):
    """The family's advance on the device — one launch of cmpc_lin_advance_dev: ``x0`` (B, nx), ``u_prev`` (B, nu)
    and ``traj_local`` (B, N+1, 2) are overwritten from ``z`` (B, nz, reference layout) for every agent whose z is
    finite (``scenarios.lin_advance``); contiguous fp64 CUDA tensors."""
    import torch

    B = int(z.shape[0])
    if z.dim() != 2 or z.shape[1] != (nx + ns) * (N + 1) + 2 * nu * N or tuple(x0.shape) != (B, nx) or \
            tuple(u_prev.shape) != (B, nu) or tuple(traj_local.shape) != (B, N + 1, _pos_dim(prm)):
        raise ValueError(f"z (B, (nx+ns)(N+1) + 2 nu N), x0 (B, nx), u_prev (B, nu), traj_local (B, N+1, {_pos_dim(prm)})")
    if B == 0:
        return
    ctx = ctx or L.default_context(z.device.index)
    if stream is None:
        stream = torch.cuda.current_stream(z.device)
    dims = L.cmpc_lin_dims(B, int(N), 0, 0, int(nx), 0)
    ctx.check(_lin_fn(ctx, prm, "advance_dev")(ctx.h, ct.byref(_lin_params(prm)), ct.byref(dims), int(ns), int(nu),
                                               _tptr(z), _tptr(x0), _tptr(u_prev), _tptr(traj_local),
                                               ct.c_void_p(getattr(stream, "cuda_stream", stream))))


def lin_publish_dev(prm, z, nx, nu, ns, N, traj_all, traj_local, atol=0.01, rtol=1e-5, self_offset=0, close=None,
                    delta=None, not_close=None, ctx=None, stream=None):
    """An inner round's publication on the device — one launch of cmpc_lin_publish_dev on ``stream`` (default:
    torch's current one), no host synchronisation; the rule is ``scenarios.lin_publish``'s, bit for bit.
    ``traj_local`` (B, N+1, 2) <- the positions predicted by ``z`` (B, nz, reference layout), or the agent's row of
    ``traj_all`` (n_total, N+1, 2) again when its z is not finite; ``close`` (B,) int32, ``delta`` (B,) fp64 and
    ``not_close`` (1,) int32 are optional: the allclose verdict against that row, the largest move, and the count
    of agents that are not close ADDED to ``not_close`` (zero it first).  Contiguous CUDA tensors; ``traj_local``
    must not alias ``traj_all``."""
    import torch

    B, pd = int(z.shape[0]), _pos_dim(prm)
    if z.dim() != 2 or z.shape[1] != (nx + ns) * (N + 1) + 2 * nu * N or traj_all.dim() != 3 or \
            tuple(traj_all.shape[1:]) != (N + 1, pd) or tuple(traj_local.shape) != (B, N + 1, pd) or \
            self_offset < 0 or self_offset + B > traj_all.shape[0]:
        raise ValueError(f"z (B, (nx+ns)(N+1) + 2 nu N), traj_all (n_total >= self_offset + B, N+1, {pd}), traj_local "
                         f"(B, N+1, {pd})")
    for name, t, dt, shp in (("close", close, torch.int32, (B,)), ("delta", delta, torch.float64, (B,)),
                             ("not_close", not_close, torch.int32, (1,))):
        if t is not None and (t.device != z.device or t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous()):
            raise ValueError(f"{name}: need a contiguous {shp} {dt} tensor on {z.device}")
    if B == 0:   # empty tensors have no address to hand over; the entry point launches nothing either
        return
    ctx = ctx or L.default_context(z.device.index)
    if stream is None:
        stream = torch.cuda.current_stream(z.device)
    dims = L.cmpc_lin_dims(B, int(N), 0, int(self_offset), int(nx), 0)
    ctx.check(_lin_fn(ctx, prm, "publish_dev")(ctx.h, ct.byref(_lin_params(prm)), ct.byref(dims), int(ns), int(nu),
                                               _tptr(z), _tptr(traj_all), float(atol), float(rtol), _tptr(traj_local),
                                               _tptr(close), _tptr(delta), _tptr(not_close),
                                               ct.c_void_p(getattr(stream, "cuda_stream", stream))))


def lpv_publish_dev(z, N, traj_all, traj_local, status=None, atol=0.01, rtol=1e-5, self_offset=0, close=None, delta=None,
                    counts=None, ctx=None, stream=None):
    """An inner round's publication of the LPV agents on the device — one launch of cmpc_lpv_publish_dev on
    ``stream`` (default: torch's current one), no host synchronisation; the rule is ``scenarios.lpv_publish``'s, bit
    for bit.  ``traj_local`` (B, N+1, 2) <- the X, Y predicted by ``z`` (B, 12(N+1) + 4N), or the agent's row of
    ``traj_all`` (n_total, N+1, 2) again when its z is not finite; ``close`` (B,) int32, ``delta`` (B,) fp64 and
    ``counts`` (2,) int32 are optional: the allclose verdict against that row, the largest move, and the counts of
    agents that are not close / infeasible by ``status`` (B,) int32 (optional) ADDED to ``counts`` (zero it first).
    Contiguous CUDA tensors; ``traj_local`` must not alias ``traj_all``."""
    import torch

    B = int(z.shape[0])
    if z.dim() != 2 or z.shape[1] != 12 * (N + 1) + 4 * N or traj_all.dim() != 3 or \
            tuple(traj_all.shape[1:]) != (N + 1, 2) or tuple(traj_local.shape) != (B, N + 1, 2) or \
            self_offset < 0 or self_offset + B > traj_all.shape[0]:
        raise ValueError("z (B, 12(N+1) + 4N), traj_all (n_total >= self_offset + B, N+1, 2), traj_local (B, N+1, 2)")
    for name, t, dt, shp in (("close", close, torch.int32, (B,)), ("delta", delta, torch.float64, (B,)),
                             ("counts", counts, torch.int32, (2,)), ("status", status, torch.int32, (B,))):
        if t is not None and (t.device != z.device or t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous()):
            raise ValueError(f"{name}: need a contiguous {shp} {dt} tensor on {z.device}")
    if B == 0:   # empty tensors have no address to hand over; the entry point launches nothing either
        return
    ctx = ctx or L.default_context(z.device.index)
    if stream is None:
        stream = torch.cuda.current_stream(z.device)
    dims = L.cmpc_di_dims(B, int(N), 0, int(self_offset))
    ctx.check(ctx.lib.cmpc_lpv_publish_dev(ctx.h, ct.byref(dims), _tptr(z), _tptr(traj_all), _tptr(status), float(atol),
                                           float(rtol), _tptr(traj_local), _tptr(close), _tptr(delta), _tptr(counts),
                                           ct.c_void_p(getattr(stream, "cuda_stream", stream))))


def lin_round_dev(prm, own, nbr, traj_all, shared, dev, out, traj_local, self_offset=0, opts=None, ctx=None,
                  stream=None):
    """One round of the family on the device (cmpc_lin_round_dev): the builder into ``dev["qlin" | "C" | "h"]``,
    cmpc_solve_mpc_batch_dev on ``dev`` (the PER_AGENT tensors of ``solver.solve_mpc_dev``) with ``shared`` (dims
    and weights) and ``opts`` (a ``_lib.opts``; None: defaults), then the advance into ``dev["x0"]``,
    ``dev["u_prev"]`` and ``traj_local``.  ``out``: dict with 'z' and optional 'kkt', 'iters', 'status'.  The
    exchange traj_local -> traj_all stays the caller's."""
    from .solver import PER_AGENT

    ctx, dims, lo, pn, st = _lin_args(traj_all, nbr, own, self_offset, ctx, stream, _pos_dim(prm))
    w, keep = _weights(shared)
    data = L.cmpc_mpc_data(*[_tptr(dev[k]) for k in PER_AGENT])
    o_ = L.cmpc_mpc_out(_tptr(out["z"]), _tptr(out.get("kkt")), _tptr(out.get("iters")), _tptr(out.get("status")))
    ctx.check(_lin_fn(ctx, prm, "round_dev")(ctx.h, ct.byref(_lin_params(prm)), ct.byref(dims), pn, ct.byref(lo),
                                             _tptr(traj_all), ct.byref(_dims(shared, dims.batch)), ct.byref(w),
                                             ct.byref(data), ct.byref(o_), None if opts is None else ct.byref(opts),
                                             _tptr(traj_local), st))
    del keep


def _lin_table_args(table, N, nbr, traj_all, mode, self_offset, ctx, stream, pd=2):
    """What the two stage-table wrappers share: the shapes read off the table's tensors (A (B, T, nx, nx), B (B, T,
    nx, nu), qlin (B, T, nx), C (B, T, mo, nx), h (B, T, mo); C / h None when mo = 0), cmpc_lin_dims,
    cmpc_lin_table_dims, cmpc_lin_table."""
    import torch

    A, Bm, q, C, h = table["A"], table["B"], table["qlin"], table.get("C"), table.get("h")
    B, T, nx = (int(v) for v in q.shape)
    nu = int(Bm.shape[3]) if Bm.dim() == 4 else -1
    mo = 0 if C is None else int(C.shape[2])
    nb = 0 if nbr is None else int(nbr.shape[1])
    if tuple(A.shape) != (B, T, nx, nx) or tuple(Bm.shape) != (B, T, nx, nu) or traj_all.dim() != 3 or \
            tuple(traj_all.shape[1:]) != (N + 1, pd) or (mo and (tuple(C.shape) != (B, T, mo, nx) or
                                                                 tuple(h.shape) != (B, T, mo))):
        raise ValueError("table: A (B, T, nx, nx), B (B, T, nx, nu), qlin (B, T, nx), C (B, T, mo, nx), h (B, T, mo); "
                         f"traj_all (n_total, N+1, {pd})")
    ctx = ctx or L.default_context(traj_all.device.index)
    if stream is None:
        stream = torch.cuda.current_stream(traj_all.device)
    dims = L.cmpc_lin_dims(B, int(N), nb, int(self_offset), nx, mo)
    tab = L.cmpc_lin_table(_tptr(A), _tptr(Bm), _tptr(q), _tptr(C) if mo else None, _tptr(h) if mo else None)
    return ctx, dims, nu, L.cmpc_lin_table_dims(T, int(mode)), tab, (_tptr(nbr) if nb and B else None), \
        ct.c_void_p(getattr(stream, "cuda_stream", stream))


def lin_table_build_dev(prm, table, t, N, nbr, traj_all, mode=L.CMPC_TABLE_HOLD, self_offset=0, out=None, ctx=None,
                        stream=None):
    """A round's whole build for agents given by a stage table — one launch of cmpc_lin_table_build_dev on
    ``stream`` (default: torch's current one), no host synchronisation: the A / B windows at time ``t``
    (``scenarios.lin_window``) and ``scenarios.lin_rows`` of that window's own data, bit for bit.  ``table``: dict
    of contiguous fp64 CUDA tensors A (B, T, nx, nx), B (B, T, nx, nu), qlin (B, T, nx), C (B, T, mo, nx), h (B, T,
    mo) (the last two None when mo = 0); ``nbr`` (B, nb) int32 (None when nb = 0); ``traj_all`` (n_total, N+1, 2).
    Writes ``out`` = (A, B, qlin, C, h) (allocated when None) and returns it."""
    import torch

    ctx, dims, nu, td, tab, pn, st = _lin_table_args(table, N, nbr, traj_all, mode, self_offset, ctx, stream,
                                                     _pos_dim(prm))
    B, N, nx, mc = dims.batch, dims.N, dims.nx, dims.mo + dims.nb
    shapes = ((B, N, nx, nx), (B, N, nx, nu), (B, N + 1, nx), (B, N, mc, nx), (B, N, mc))
    if out is None:
        out = tuple(torch.empty(shp, dtype=torch.float64, device=traj_all.device) for shp in shapes)
    if tuple(tuple(o.shape) for o in out) != shapes:
        raise ValueError("out: A (B, N, nx, nx), B (B, N, nx, nu), qlin (B, N+1, nx), C (B, N, mo+nb, nx), h (B, N, mo+nb)")
    if B == 0:   # empty tensors have no address to hand over; the entry point launches nothing either
        return out
    # (no rows at all: C and h are empty and never written; the entry point still wants an address)
    spare = torch.empty(1, dtype=torch.float64, device=traj_all.device) if mc == 0 else None
    ctx.check(_lin_fn(ctx, prm, "table_build_dev")(ctx.h, ct.byref(_lin_params(prm)), ct.byref(dims), nu, ct.byref(td),
                                                   ct.byref(tab), int(t), pn, _tptr(traj_all),
                                                   *[_tptr(o if o.numel() else spare) for o in out], st))
    return out


def lin_table_round_dev(prm, table, t, nbr, traj_all, shared, dev, out, traj_local, mode=L.CMPC_TABLE_HOLD,
                        self_offset=0, opts=None, ctx=None, stream=None):
    """One round of stage-table agents on the device (cmpc_lin_table_round_dev): ``lin_table_build_dev`` at time
    ``t`` into ``dev["A" | "B" | "qlin" | "C" | "h"]``, then as ``lin_round_dev``: the solver on ``dev`` with
    ``shared`` and ``opts``, the advance into ``dev["x0"]``, ``dev["u_prev"]`` and ``traj_local``.  Moving ``t`` on
    and the exchange stay the caller's."""
    from .solver import PER_AGENT

    ctx, dims, nu, td, tab, pn, st = _lin_table_args(table, int(shared["N"]), nbr, traj_all, mode, self_offset, ctx,
                                                     stream, _pos_dim(prm))
    w, keep = _weights(shared)
    data = L.cmpc_mpc_data(*[_tptr(dev[k]) for k in PER_AGENT])
    o_ = L.cmpc_mpc_out(_tptr(out["z"]), _tptr(out.get("kkt")), _tptr(out.get("iters")), _tptr(out.get("status")))
    ctx.check(_lin_fn(ctx, prm, "table_round_dev")(ctx.h, ct.byref(_lin_params(prm)), ct.byref(dims), pn, ct.byref(td),
                                                   ct.byref(tab), int(t), _tptr(traj_all),
                                                   ct.byref(_dims(shared, dims.batch)), ct.byref(w), ct.byref(data),
                                                   ct.byref(o_), None if opts is None else ct.byref(opts),
                                                   _tptr(traj_local), st))
    del keep


def _di_params(p):
    """cmpc_di_params of a scenario's ``params``."""
    return L.cmpc_di_params(int(p["dim"]), *(float(p[k]) for k in ("v_ref", "q_v", "q_lane", "hw", "min_vel", "max_vel",
                                                                     "min_dist", "wq")))


def _di_opts(tol, max_iter, fp32):
    """The synthetic family's cmpc_opts: fp32 selects CMPC_FLAG_FP32 and, without ``tol``, FP32_TOL."""
    from .solver import FP32_TOL

    return L.opts(tol or (FP32_TOL if fp32 else None), max_iter, L.CMPC_FLAG_FP32 if fp32 else 0)


def _lpt_default(sh, N, fp32):
    """Whether the agents are launched longest-first, by last round's IPM iterations (cmpc_opts.order), when the
    caller does not say: on where the stage-wise Riccati solver runs (many agents per SIMD there, so the launch
    otherwise ends with whichever slow agents happened to start last; the condensed kernels have one agent per
    SIMD and ignore the order).  The fp32 lane kernel packs its wavefronts in that order, but at cfg5 all of its
    256 wavefronts run at once (one per CU), so its launch still ends with the slowest agent (measured 91.9 ->
    99.8 ms): off where fp32 runs on it, i.e. on dimensions without the Riccati kernel's fp32 instantiation
    (6, 3, 6)."""
    ric32 = (sh["nx"], sh["nu"], sh["mc"]) == (6, 3, 6)
    return N * sh["nu"] > 64 and (not fp32 or ric32)


def is_lti(A, B):
    """Whether the agents' models are time-invariant in the sense of CMPC_FLAG_LTI: ``A`` (batch, N, nx, nx) and
    ``B`` (batch, N, nx, nu) are fp64, every stage of an agent is bit-equal to its stage 0 (compared as 64-bit
    patterns: -0.0 is not +0.0) and every entry is finite.  The test ``cmpc_di_rounds_create`` runs on its
    host arrays."""
    for M in (A, B):
        M = np.ascontiguousarray(M, dtype=np.float64)
        if M.ndim != 4 or not np.isfinite(M).all():
            return False
        bits = M.view(np.uint64)
        if not (bits == bits[:, :1]).all():
            return False
    return True


class _TorchRounds:
    """What the torch-driven ``DIRounds`` / ``LPVRounds`` share; they set ``torch``, ``dev``, ``ctx``, the shard
    (``B``, ``off``, ``nb``, ``world``, ``group``, ``comm``), ``traj_all`` / ``traj_local`` / ``nbr`` and
    ``reselect_window``."""

    def _stream(self):
        return ct.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def exchange(self):
        exchange_positions(self.traj_all, self.traj_local, self.world, self.group, self.comm)

    def select_neighbours(self, window=None):
        """One selection into ``self.nbr``, in place: this rank's agents against the exchange buffer as it
        stands (``select_neighbours_dev``; ``window`` defaults to ``reselect_window``)."""
        select_neighbours_dev(self.traj_all, self.nb, self.B, self.off, self.reselect_window if window is None
                              else window, out=self.nbr, ctx=self.ctx)


class _RoundsHandle:
    """What the round-handle wrappers share (cmpc_lpv_rounds_* / cmpc_di_rounds_* / cmpc_lin_rounds_*): the
    handle's lifetime, the host exchange and the device log.  A wrapper sets ``_fn`` (the entry points' common
    prefix), ``ctx``, ``B``, ``n``, ``N`` and ``nx`` / ``nu`` (the widths of the log's state and input rows)."""

    def _call(self, name, *args):
        self.ctx.check(getattr(self.ctx.lib, self._fn + name)(self.h, *args))

    @staticmethod
    def _flags(host_exchange=False, halt=True, reselect=False, lpt=False):
        return (L.CMPC_ROUNDS_HOST_EXCHANGE if host_exchange else 0) | (0 if halt else L.CMPC_ROUNDS_NO_HALT) | \
            (L.CMPC_ROUNDS_RESELECT if reselect else 0) | (L.CMPC_ROUNDS_LPT if lpt else 0)

    def _create(self, args, log, log_separation, create="create"):
        """<prefix><create>(ctx, *args, &h), then the log (``log`` = capacity)."""
        h = ct.c_void_p()
        create = getattr(self.ctx.lib, self._fn + create)
        self.ctx.check(create(self.ctx.h, *[ct.byref(a) for a in args], ct.byref(h)))
        self.h = h
        self.log_separation = bool(log_separation)
        if log or log_separation:
            self._call("log_enable", int(log), L.CMPC_LOG_SEPARATION if log_separation else 0)

    pd = 2   # coordinates of a position: 3 on a linear-model handle whose ``prm`` has ``iz``

    def get_traj(self):
        t = np.zeros((self.B, self.N + 1, self.pd))
        self._call("get_traj", L.dptr(t))
        return t

    def set_traj(self, traj_all):
        t = L.f64(traj_all)
        if t.shape != (self.n, self.N + 1, self.pd):
            raise ValueError(f"traj_all: (n_total, N+1, {self.pd})")
        self._call("set_traj", L.dptr(t))

    def close(self):
        if getattr(self, "h", None):
            getattr(self.ctx.lib, self._fn + "destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def consensus(self):
        """The latest consensus step (the handles that have ``step_consensus``): dict of inner_rounds, agreed (bool),
        not_close (inner_rounds,) int32 — the node-wide count of agents whose published positions moved, after each
        inner round (entry 0: against the previous step's plan) — and this rank's close (B,) int32 and delta (B,) of
        the last inner round."""
        n, agreed = ct.c_int(), ct.c_int()
        o = L.cmpc_consensus_out(ct.pointer(n), ct.pointer(agreed), None, 0, None, None)
        self._call("consensus_read", ct.byref(o))
        r = dict(inner_rounds=n.value, agreed=bool(agreed.value), not_close=np.zeros(n.value, np.int32),
                 close=np.zeros(self.B, np.int32), delta=np.zeros(self.B))
        o = L.cmpc_consensus_out(None, None, L.iptr(r["not_close"]) if n.value else None, n.value, L.iptr(r["close"]),
                                 L.dptr(r["delta"]))
        self._call("consensus_read", ct.byref(o))
        return r

    def log_range(self):
        """(first, count): the rounds the log ring holds now, counted from create."""
        first, count = ct.c_int(), ct.c_int()
        self._call("log_range", ct.byref(first), ct.byref(count))
        return first.value, count.value

    def log(self, first=None, count=None):
        """Rounds [first, first + count) of the log (default: everything the ring holds) as a dict of arrays with
        leading dimension ``count``: state (count, B, nx) = xPred[0], u (count, B, nu) = uPred[0], look_ahead,
        kkt, iters, status (count, B), solve_ms (count,): the whole batch's solver launch of the round, in
        milliseconds; with ``log_separation`` nearest (count, B) int32, each agent's nearest other agent after
        the round's exchange, and sep2 the squared distance.  ``logio.save_run`` writes it as the reference's
        csv/<id>/*.dat.  A round outside the ring raises CmpcError(CMPC_ERR_ARG)."""
        if first is None or count is None:
            lo, n = self.log_range()
            first = lo if first is None else first
            count = lo + n - first if count is None else count
        c = max(int(count), 0)
        r = dict(state=np.zeros((c, self.B, self.nx)), u=np.zeros((c, self.B, self.nu)),
                 look_ahead=np.zeros((c, self.B)), kkt=np.zeros((c, self.B)), iters=np.zeros((c, self.B), np.int32),
                 status=np.zeros((c, self.B), np.int32), solve_ms=np.zeros(c))
        if self.log_separation:
            r.update(sep2=np.zeros((c, self.B)), nearest=np.zeros((c, self.B), np.int32))
        o = L.cmpc_rounds_log(L.dptr(r["state"]), L.dptr(r["u"]), L.dptr(r["look_ahead"]), L.dptr(r["kkt"]),
                              L.iptr(r["iters"]), L.iptr(r["status"]), L.dptr(r.get("sep2")), L.iptr(r.get("nearest")),
                              L.dptr(r["solve_ms"]))
        self._call("log_read", int(first), int(count), ct.byref(o))
        return r


class DIRounds(_TorchRounds):
    """Device-resident consensus rounds of the synthetic double-integrator agents (module docstring).

    ``reselect`` = r > 0: the neighbour table ``self.nbr`` is re-selected on the device, in place, at the
    start of ``step()`` on rounds 0, r, 2r, ... (``select_neighbours_dev`` with ``reselect_window``, on the
    round's stream, before the rows are built), so the collision rows and the coverage term follow the agents
    that are nearest now instead of those of the scenario's t = 0 table.  0 (the default): the table stays
    what the scenario gave, and ``step()`` is launch for launch what it was.  Selected neighbours come nearest
    first, not in the reference's index order of ns[i]; only the order of an agent's collision rows follows.

    ``lti``: CMPC_FLAG_LTI, the promise that every stage of an agent's A and B equals its stage 0 (the fused
    round then tabulates the condensed dynamics once per solve, same bits).  None (the default): set when
    ``is_lti`` finds it so on this rank's ``scen.A``, ``scen.B``; False: never; True: set without the test."""

    def __init__(self, scen, rank=0, world=1, device=None, ctx=None, tol=None, max_iter=None, group=None,
                 fp32=False, comm=None, fused=True, lpt=None, reselect=0, reselect_window=(0, 0), lti=None):
        import torch

        self.torch = torch
        self.scen, self.rank, self.world, self.group, self.comm = scen, rank, world, group, comm
        # step(): rows built, and the round advanced, inside the solver launch (cmpc_di_round_dev) instead
        # of build() + solve() + advance()
        self.fused = fused
        self.reselect, self.reselect_window, self.rounds_done = int(reselect), tuple(reselect_window), 0
        if scen.n_agents % world:
            raise ValueError("n_agents must be divisible by the number of ranks")
        self.dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.ctx = ctx or L.default_context(self.dev.index)
        sl = scen.shard(rank, world)
        self.off = sl.start
        self.B = sl.stop - sl.start
        self.N, self.nb = scen.N, scen.nb
        sh = scen.shared
        self.shared = sh
        T = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.dev)
        self.A = T(scen.A[sl])
        self.Bm = T(scen.B[sl])
        self.x0 = T(scen.x0[sl])
        self.u_prev = T(scen.u_prev[sl])
        self.lane = T(scen.lane[sl])
        self.nbr = T(scen.nbr[sl], torch.int32)
        self.traj_all = T(scen.traj)
        self.traj_local = torch.empty((self.B, self.N + 1, 2), dtype=torch.float64, device=self.dev)
        nx, mc = sh["nx"], sh["mc"]
        self.qlin = torch.empty((self.B, self.N + 1, nx), dtype=torch.float64, device=self.dev)
        self.C = torch.empty((self.B, self.N, mc, nx), dtype=torch.float64, device=self.dev)
        self.h = torch.empty((self.B, self.N, mc), dtype=torch.float64, device=self.dev)
        self.z = torch.empty((self.B, nz_of(sh)), dtype=torch.float64, device=self.dev)
        self.kkt = torch.empty(self.B, dtype=torch.float64, device=self.dev)
        self.iters = torch.empty(self.B, dtype=torch.int32, device=self.dev)
        self.status = torch.empty(self.B, dtype=torch.int32, device=self.dev)
        self.dprm = _di_params(scen.params)
        self.ddims = L.cmpc_di_dims(self.B, self.N, self.nb, self.off)
        self.mdims = _dims(sh, self.B)
        self.w, self._wkeep = _weights(sh)
        self.opts = _di_opts(tol, max_iter, fp32)
        # CMPC_FLAG_LTI: set when this rank's A, B pass is_lti (None), never (False) or untested (True)
        self.lti = is_lti(scen.A[sl], scen.B[sl]) if lti is None else bool(lti)
        if self.lti:
            self.opts.flags |= L.CMPC_FLAG_LTI
        self.lpt = _lpt_default(sh, self.N, fp32) if lpt is None else bool(lpt)   # cmpc_opts.order
        self._order = None
        self.data = L.cmpc_mpc_data(*[_tptr(t) for t in (self.A, self.Bm, self.x0, self.u_prev, self.qlin,
                                                          self.C, self.h)])
        self.out = L.cmpc_mpc_out(_tptr(self.z), _tptr(self.kkt), _tptr(self.iters), _tptr(self.status))

    def bind_outputs(self, kkt, iters, status):
        """Point the solver's per-agent kkt / iters / status outputs at other (B,) device
        tensors (e.g. one row per round of a preallocated history), without copies."""
        torch = self.torch
        for name, t, dt in (("kkt", kkt, torch.float64), ("iters", iters, torch.int32),
                            ("status", status, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.device != self.dev or t.dtype != dt or \
                    tuple(t.shape) != (self.B,) or not t.is_contiguous():
                raise ValueError(f"{name}: need a contiguous ({self.B},) {dt} tensor on {self.dev}")
        self.kkt, self.iters, self.status = kkt, iters, status
        self.out = L.cmpc_mpc_out(_tptr(self.z), _tptr(kkt), _tptr(iters), _tptr(status))

    def build(self):
        lib = self.ctx.lib
        self.ctx.check(lib.cmpc_di_build_dev(self.ctx.h, ct.byref(self.dprm), ct.byref(self.ddims), _tptr(self.nbr),
                                             _tptr(self.lane), _tptr(self.traj_all), _tptr(self.qlin),
                                             _tptr(self.C), _tptr(self.h), self._stream()))

    def _order_in(self):
        self.opts.order = self._order.data_ptr() if (self.lpt and self._order is not None) else None

    def _order_out(self):
        if self.lpt:  # next round's launch order (stream-ordered after this solve)
            self._order = self.torch.argsort(self.iters, descending=True, stable=True).to(self.torch.int32)

    def solve(self):
        self._order_in()
        self.ctx.check(self.ctx.lib.cmpc_solve_mpc_batch_dev(self.ctx.h, ct.byref(self.mdims), ct.byref(self.w),
                                                             ct.byref(self.data), ct.byref(self.out),
                                                             ct.byref(self.opts), self._stream()))
        self._order_out()

    def build_solve(self):
        """build() + solve() as one launch where the v3 kernel covers the problem (the rows go
        from traj_all straight into the solver's LDS, bit-identical to build()); qlin / C / h are
        then left untouched — call build() before snapshot() to materialise them."""
        lib = self.ctx.lib
        self._order_in()
        self.ctx.check(lib.cmpc_di_solve_dev(self.ctx.h, ct.byref(self.dprm), ct.byref(self.ddims), _tptr(self.nbr),
                                             _tptr(self.lane), _tptr(self.traj_all), ct.byref(self.mdims),
                                             ct.byref(self.w), ct.byref(self.data), ct.byref(self.out),
                                             ct.byref(self.opts), self._stream()))
        self._order_out()

    def round(self):
        """build_solve() + advance() as one call (cmpc_di_round_dev): where the v3 kernel covers the
        problem the solver's launch also writes x0 <- x_1, u_prev <- u_0 and traj_local (the same
        values advance() reads back from z), one launch less per round."""
        lib = self.ctx.lib
        self._order_in()
        self.ctx.check(lib.cmpc_di_round_dev(self.ctx.h, ct.byref(self.dprm), ct.byref(self.ddims), _tptr(self.nbr),
                                             _tptr(self.lane), _tptr(self.traj_all), ct.byref(self.mdims),
                                             ct.byref(self.w), ct.byref(self.data), ct.byref(self.out),
                                             ct.byref(self.opts), _tptr(self.traj_local), self._stream()))
        self._order_out()

    def advance(self):
        self.ctx.check(self.ctx.lib.cmpc_di_advance_dev(self.ctx.h, ct.byref(self.dprm), ct.byref(self.ddims),
                                                        _tptr(self.z), _tptr(self.x0), _tptr(self.u_prev),
                                                        _tptr(self.traj_local), self._stream()))

    def step(self, timer=None):
        """One consensus round.  `timer` (start, stop) events bracket the solve launch (with
        `fused`, the launch that builds and solves)."""
        if self.reselect > 0 and self.nb and self.rounds_done % self.reselect == 0:
            self.select_neighbours()
        self.rounds_done += 1
        if not self.fused:
            self.build()
        if timer is not None:
            timer[0].record()
        if self.fused:
            self.round()
        else:
            self.solve()
        if timer is not None:
            timer[1].record()
        if not self.fused:
            self.advance()
        self.exchange()

    def snapshot(self):
        """Host copy of this rank's current structured problem (for checkers)."""
        p = dict(self.shared)
        for k, t in (("A", self.A), ("B", self.Bm), ("x0", self.x0), ("u_prev", self.u_prev), ("qlin", self.qlin),
                     ("C", self.C), ("h", self.h)):
            p[k] = t.detach().cpu().numpy().copy()
        return p


class LPVRounds(_TorchRounds):
    """Device-resident consensus rounds of the reference's LPV agents (LPV_HP_N_main.py:96-117):
    per round gather (neighbour and own positions from the exchange buffer) -> build + solve
    (cmpc_solve_lpv_batch_dev: scheduling, planes, weights, rows, the QP) -> advance (x0 <-
    xPred[1], Last_xPredicted <- xPred[1:], uPred, [OldSteering, OldAccelera] <- u_0) -> exchange
    (all-gather of the predicted X, Y).  Everything stays in HBM; the host only launches.

    ``bp``: a ``PlannerLPVBatch`` (gains, map, horizon, options, context).  Population arrays
    (all ranks' agents, sharded contiguously): x0 (n, 9), x_last (n, N+1, 9) (the first
    round's Last_xPredicted), u_last (n, N, 2), nbr (n, nb) neighbour indices (the reference: all
    other agents, :82-85), u_old (n, 2) (default 0, PlannerLPV's initial OldSteering /
    OldAccelera), traj (n, N+1, 2) (default x_last[:, :, 7:9], the reference's initial
    ``agents``).

    ``reselect`` = r > 0 (with ``reselect_window``): ``nbr`` is only the table's first content — at the start
    of ``step()`` on rounds 0, r, 2r, ... the table is re-selected on the device, in place
    (``select_neighbours_dev``, before the gather, on the round's stream).  The default 0 keeps the table for
    good, as the reference.  Selected neighbours come nearest first, not in the reference's index order of
    ns[i]: the order of an agent's collision rows and of the ``planes`` columns follows."""

    def __init__(self, bp, x0, x_last, u_last, nbr, u_old=None, traj=None, rank=0, world=1, group=None, comm=None,
                 reselect=0, reselect_window=(0, 0)):
        import torch

        self.torch, self.bp, self.ctx = torch, bp, bp.ctx
        self.rank, self.world, self.group, self.comm = rank, world, group, comm
        self.reselect, self.reselect_window, self.rounds_done = int(reselect), tuple(reselect_window), 0
        x0 = np.asarray(x0, np.float64)
        n, N = x0.shape[0], bp.N
        if n % world:
            raise ValueError("agents must be divisible by the number of ranks")
        nbr = np.asarray(nbr, np.int32).reshape(n, -1)
        if nbr.size and (nbr.min() < 0 or nbr.max() >= n):
            raise ValueError("nbr: neighbour indices must address the population (0 <= j < n)")
        if np.shape(u_last) != (n, N, 2) or (u_old is not None and np.shape(u_old) != (n, 2)) or \
                (traj is not None and np.shape(traj) != (n, N + 1, 2)) or x0.shape != (n, 9):
            raise ValueError("x0 (n, 9), u_last (n, N, 2), u_old (n, 2), traj (n, N+1, 2) expected")
        self.N, self.nb = N, nbr.shape[1]
        self.B = n // world
        sl = slice(rank * self.B, (rank + 1) * self.B)
        self.off = sl.start
        self.dev = torch.device("cuda", self.ctx.device)
        T = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.dev)  # noqa
        x_last = np.asarray(x_last, np.float64)
        if x_last.shape != (n, N + 1, 9):   # the gather / builder kernels trust these extents
            raise ValueError("x_last: the first round's Last_xPredicted, (n, N+1, 9)")
        self.x0 = T(x0[sl])
        self.x_last = T(x_last[sl])
        self.u_last = T(np.asarray(u_last, np.float64)[sl])
        self.u_old = T(np.zeros((n, 2)) if u_old is None else np.asarray(u_old, np.float64))[sl].contiguous()
        self.nbr = T(nbr[sl], torch.int32)
        self.traj_all = T(x_last[:, :, 7:9] if traj is None else traj)
        # this rank's rows of the exchange buffer; an agent that is not advanced (no finite
        # solution) keeps them, so they start as the initial trajectories
        self.traj_local = self.traj_all[sl].clone()
        self.pose = torch.empty((self.B, N + 1, 2), dtype=torch.float64, device=self.dev)
        self.x_agents = torch.empty((self.B, N + 1, max(self.nb, 1), 2), dtype=torch.float64, device=self.dev)
        nz = 12 * (N + 1) + 4 * N
        self.z = torch.empty((self.B, nz), dtype=torch.float64, device=self.dev)
        self.planes = torch.zeros((self.B, N, 3, max(self.nb, 1)), dtype=torch.float64, device=self.dev)
        self.kkt = torch.empty(self.B, dtype=torch.float64, device=self.dev)
        self.iters = torch.empty(self.B, dtype=torch.int32, device=self.dev)
        self.status = torch.empty(self.B, dtype=torch.int32, device=self.dev)
        self.last_rows = N + 1
        self.rdims = L.cmpc_di_dims(self.B, N, self.nb, self.off)
        # agents of the latest round the reference calls infeasible (status not in {1, 2, -2})
        self.n_infeasible = torch.zeros(1, dtype=torch.int32, device=self.dev)
        # the latest consensus step (step_consensus): the last inner round's verdicts and its two counts (not close,
        # infeasible) on the device, the node-wide not-close count of every inner round and the loop's outcome
        self.close = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self.delta = torch.zeros(self.B, dtype=torch.float64, device=self.dev)
        self.counts = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self.trace, self.agreed = [], False

    def gather(self):
        lib = self.ctx.lib
        self.ctx.check(lib.cmpc_lpv_gather_dev(self.ctx.h, ct.byref(self.rdims), _tptr(self.nbr), _tptr(self.traj_all),
                                               _tptr(self.x_agents) if self.nb else None, _tptr(self.pose),
                                               self._stream()))

    def solve(self):
        lib, bp = self.ctx.lib, self.bp
        dims = L.cmpc_lpv_dims(self.B, self.N, self.nb, self.last_rows)
        data = L.cmpc_lpv_data(_tptr(self.x0), _tptr(self.x_last), _tptr(self.u_last), _tptr(self.u_old),
                               _tptr(self.x_agents) if self.nb else None, _tptr(self.pose))
        out = L.cmpc_lpv_out(_tptr(self.z), _tptr(self.planes) if self.nb else None, _tptr(self.kkt),
                             ct.cast(self.iters.data_ptr(), L._IP), ct.cast(self.status.data_ptr(), L._IP))
        self.ctx.check(lib.cmpc_solve_lpv_batch_dev(self.ctx.h, ct.byref(bp.prm), ct.byref(bp.track), ct.byref(dims),
                                                    ct.byref(data), ct.byref(out), ct.byref(bp.opts),
                                                    self._stream()))

    def advance(self):
        """x0 <- xPred[1], Last_xPredicted <- xPred[1:], uPred, u_old <- u_0, the exchanged X, Y; an agent
        without a finite solution keeps its state and trajectory; infeasible agents are counted."""
        self.n_infeasible.zero_()
        if self.last_rows == self.N + 1:
            # first round: Last_xPredicted goes from N + 1 rows per agent to N dense rows.  An agent the
            # advance leaves alone (no finite solution) must find its own previous rows in its dense
            # slot, not bytes of the (N + 1)-row layout: compact the layout first (rows 0..N-1)
            dense = self.x_last[:, :self.N, :].contiguous()
            self.x_last.view(-1)[:dense.numel()].copy_(dense.view(-1))
        self.ctx.check(self.ctx.lib.cmpc_lpv_advance_dev(self.ctx.h, ct.byref(self.rdims), _tptr(self.z),
                                                         _tptr(self.x0), _tptr(self.x_last), _tptr(self.u_last),
                                                         _tptr(self.u_old), _tptr(self.traj_local),
                                                         _tptr(self.status), _tptr(self.n_infeasible),
                                                         self._stream()))
        self.last_rows = self.N   # x_old = xPred[1:] from now on (LPV_HP_N_main.py:115)

    def step(self, timer=None, halt=True):
        """One consensus round.  `timer` (start, stop) events bracket the build + solve launch.
        ``halt``: like the reference (LPV_HP_N_main.py:102-111, "QUIT..."), raise InfeasibleRound when an
        agent of this rank is infeasible (reads a device counter: one host synchronisation per round;
        ``halt=False`` leaves the check to the caller, ``infeasible()``)."""
        if self.reselect > 0 and self.nb and self.rounds_done % self.reselect == 0:
            self.select_neighbours()
        self.rounds_done += 1
        self.gather()
        if timer is not None:
            timer[0].record()
        self.solve()
        if timer is not None:
            timer[1].record()
        self.advance()
        self.exchange()
        if halt:
            bad = self.infeasible_all()
            if bad:
                raise InfeasibleRound(bad)

    def infeasible(self):
        """Infeasible agents of this rank in the latest round (synchronises)."""
        return int(self.n_infeasible.item())

    def infeasible_all(self):
        """Infeasible agents of every rank in the latest round (synchronises; collective when
        sharded).  The reference's loop quits for every agent at once (LPV_HP_N_main.py:102-111):
        each rank takes the halt decision on the node's count, so no rank breaks out of the loop
        while the others wait for it in the next round's all-gather."""
        return self._node_sum(self.n_infeasible)[0]

    def _node_sum(self, counts):
        """The int32 device counters ``counts`` summed over every rank, as a list of ints (synchronises; collective
        when sharded)."""
        if self.world == 1:
            return counts.tolist()
        cnt = counts.clone()
        if self.comm is not None:   # libcmpc's RCCL communicator (cmpc_comm_sum_i32)
            self.comm.sum_i32(cnt, self.torch.cuda.current_stream(self.dev))
            return cnt.tolist()
        import torch.distributed as dist

        if dist.get_backend(self.group) == "gloo":   # gloo reduces host tensors
            cnt = cnt.cpu()
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=self.group)
        return cnt.tolist()

    def publish(self, atol=0.01, rtol=1e-5):
        """An inner round's publication (``lpv_publish_dev``): ``traj_local`` <- the predicted X, Y, ``close`` /
        ``delta`` against this rank's rows of the exchange buffer, ``counts`` <- this rank's (not close, infeasible).
        Nothing else moves: x0, x_last, u_last, u_old stay the step's."""
        self.counts.zero_()
        lpv_publish_dev(self.z, self.N, self.traj_all, self.traj_local, status=self.status, atol=atol, rtol=rtol,
                        self_offset=self.off, close=self.close, delta=self.delta, counts=self.counts, ctx=self.ctx)

    def step_consensus(self, min_rounds=3, need=2, max_rounds=12, atol=0.01, rtol=1e-5, halt=True):
        """One consensus step (what cmpc_lpv_rounds_step_consensus runs): gather, solve, publish and exchange are
        repeated at the step's state AND linearisation (x0, x_last, u_last, u_old: every inner round linearises
        about the previous step's prediction, as a plain round does; only the planes and the coverage weights are
        re-cut against the newly published positions) until the published positions agree — the rule of
        ``scenarios.consensus_stop`` on the node-wide counts — and then advances once.  An infeasible agent ends the
        inner loop after its round when ``halt``, and InfeasibleRound is raised after the step has completed, as
        ``step()`` does.  One host synchronisation per inner round.  Leaves ``trace`` (the node-wide not-close count
        after each inner round), ``agreed``, ``close`` and ``delta``; returns (inner rounds, agreed)."""
        from .scenarios import consensus_stop

        if min_rounds < 1 or need < 1 or max_rounds < min_rounds or not (atol >= 0 and rtol >= 0):
            raise ValueError("step_consensus: 1 <= min_rounds <= max_rounds, need >= 1, atol, rtol >= 0")
        if self.reselect > 0 and self.nb and self.rounds_done % self.reselect == 0:
            self.select_neighbours()
        self.rounds_done += 1
        trace = []
        while True:
            self.gather()
            self.solve()
            self.publish(atol, rtol)
            self.exchange()
            not_close, bad = self._node_sum(self.counts)
            trace.append(not_close)
            stop, agreed = consensus_stop(trace, min_rounds, need, max_rounds)
            if stop or (halt and bad):
                break
        self.advance()   # traj_local again, with the values the last inner round exchanged: no second exchange
        self.trace, self.agreed = trace, agreed
        if halt and bad:
            raise InfeasibleRound(bad)
        return len(trace), agreed


class InfeasibleRound(RuntimeError):
    """A round left agents infeasible (status not in {1, 2, -2}, LPV_Planner.py:243-249); the
    reference stops the experiment there (LPV_HP_N_main.py:102-111)."""

    def __init__(self, count):
        super().__init__(f"{count} agent(s) infeasible in this round: QUIT (LPV_HP_N_main.py:102-111)")
        self.count = count


class LPVRoundsHandle(_RoundsHandle):
    """The same rounds through the C ABI's round handle (cmpc_lpv_rounds_*): the library owns the
    device state; no torch.  What a MATLAB (MEX) or C host drives.  Arguments as LPVRounds;
    ``host_exchange``: the caller exchanges positions between steps (get_traj / set_traj).  ``reselect``:
    CMPC_ROUNDS_RESELECT — every round starts with the (0, 0) neighbour selection on the handle's exchange
    buffer (``nbr`` is only the table's first content), as ``LPVRounds(reselect=1)``.  ``log`` = capacity > 0:
    the device log of the last ``capacity`` rounds (cmpc_lpv_rounds_log_enable; ``log_range()``, ``log()``),
    with ``log_separation`` also each agent's nearest other agent; 0 (the default): off, every launch as before."""

    _fn, nx, nu = "cmpc_lpv_rounds_", 9, 2

    def __init__(self, bp, x0, x_last, u_last, nbr, u_old=None, traj=None, rank=0, world=1, host_exchange=False,
                 halt=True, reselect=False, log=0, log_separation=False):
        self.bp, self.ctx = bp, bp.ctx
        x0 = L.f64(x0)
        n, N = x0.shape[0], bp.N
        nbr = L.i32(np.asarray(nbr).reshape(n, -1))
        if n % world:
            raise ValueError("agents must be divisible by the number of ranks")
        B = n // world
        sl = slice(rank * B, (rank + 1) * B)
        self.N, self.nb, self.B, self.n = N, nbr.shape[1], B, n
        self.dims = L.cmpc_lpv_rounds_dims(n, B, rank * B, N, self.nb, self._flags(host_exchange, halt, reselect))
        keep = [L.f64(x0[sl]), L.f64(np.asarray(x_last)[sl]), L.f64(np.asarray(u_last)[sl]),
                None if u_old is None else L.f64(np.asarray(u_old)[sl]), L.i32(nbr[sl]),
                None if traj is None else L.f64(traj)]
        init = L.cmpc_lpv_rounds_init(L.dptr(keep[0]), L.dptr(keep[1]), L.dptr(keep[2]), L.dptr(keep[3]),
                                      L.iptr(keep[4]), L.dptr(keep[5]))
        self._create((bp.prm, bp.track, self.dims, init, bp.opts), log, log_separation)

    def step(self, rounds=1):
        """Runs up to `rounds` rounds; returns (rounds done, infeasible agents of the last one)."""
        done, bad = ct.c_int(), ct.c_int()
        self._call("step", int(rounds), ct.byref(done), ct.byref(bad))
        return done.value, bad.value

    def step_consensus(self, steps=1, min_rounds=3, need=2, max_rounds=12, atol=0.01, rtol=1e-5):
        """Runs up to ``steps`` consensus steps (cmpc_lpv_rounds_step_consensus), each what
        ``LPVRounds.step_consensus`` runs: gather, solve, publish and exchange repeated at the handle's state and
        linearisation until the published positions agree, then one advance.  A consensus step is one round for
        ``log``; ``max_rounds=1`` is ``step(1)``.  With ``halt`` (the default at create) an infeasible agent ends its
        step's inner loop and the call.  Returns (steps done, inner rounds run, infeasible agents of the last inner
        round); ``consensus()`` has the trace."""
        co = L.cmpc_consensus_opts(int(min_rounds), int(need), int(max_rounds), float(atol), float(rtol))
        done, inner, bad = ct.c_int(), ct.c_int(), ct.c_int()
        self._call("step_consensus", int(steps), ct.byref(co), ct.byref(done), ct.byref(inner), ct.byref(bad))
        return done.value, inner.value, bad.value

    def read(self):
        nz = 12 * (self.N + 1) + 4 * self.N
        r = dict(z=np.zeros((self.B, nz)), kkt=np.zeros(self.B), iters=np.zeros(self.B, np.int32),
                 status=np.zeros(self.B, np.int32), x0=np.zeros((self.B, 9)),
                 planes=np.zeros((self.B, self.N, 3, self.nb)))
        o = L.cmpc_lpv_rounds_out(L.dptr(r["z"]), L.dptr(r["kkt"]), L.iptr(r["iters"]), L.iptr(r["status"]),
                                  L.dptr(r["x0"]), L.dptr(r["planes"]) if self.nb else None)
        self._call("read", ct.byref(o))
        return r


class DIRoundsHandle(_RoundsHandle):
    """``DIRounds.step()`` (fused) through the C ABI's round handle (cmpc_di_rounds_*): the library owns the
    device state; no torch.  What a MATLAB (MEX) or C host drives for the synthetic family.  ``scen``: a
    ``scenarios.DIScenario``; ``rank`` / ``world``: this handle's contiguous shard, exchanged over the
    context's communicator or, with ``host_exchange``, by the caller between steps (get_traj / set_traj).
    ``reselect``: CMPC_ROUNDS_RESELECT, as ``DIRounds(reselect=1)``.  ``lpt``: CMPC_ROUNDS_LPT, the launch
    order from the previous round's iteration counts on the device (None: ``DIRounds``'s default rule).
    ``history``: rounds of kkt / iters / status the device ring keeps (``history()``).  ``log`` = capacity > 0:
    the device log of the last ``capacity`` rounds (cmpc_di_rounds_log_enable; ``log_range()``, ``log()``), with
    ``log_separation`` also each agent's nearest other agent; 0 (the default): off, every launch as before."""

    _fn = "cmpc_di_rounds_"

    def __init__(self, scen, rank=0, world=1, ctx=None, tol=None, max_iter=None, fp32=False, host_exchange=False,
                 reselect=False, lpt=None, history=1, log=0, log_separation=False):
        if scen.n_agents % world:
            raise ValueError("n_agents must be divisible by the number of ranks")
        self.ctx = ctx or L.default_context(0)
        sl = scen.shard(rank, world)
        sh = scen.shared
        self.B, self.n, self.N, self.nb = sl.stop - sl.start, scen.n_agents, scen.N, scen.nb
        self.nx, self.nu, self.nz = sh["nx"], sh["nu"], nz_of(sh)
        self.lpt = _lpt_default(sh, self.N, fp32) if lpt is None else bool(lpt)
        flags = self._flags(host_exchange, reselect=reselect, lpt=self.lpt)
        self.dims = L.cmpc_di_rounds_dims(self.n, self.B, sl.start, self.N, self.nb, flags, int(history))
        w, wkeep = _weights(sh)
        keep = [L.f64(scen.A[sl]), L.f64(scen.B[sl]), L.f64(scen.x0[sl]), L.f64(scen.u_prev[sl]), L.f64(scen.lane[sl]),
                L.i32(scen.nbr[sl]), L.f64(scen.traj)]
        init = L.cmpc_di_rounds_init(*[L.dptr(a) for a in keep[:5]], L.iptr(keep[5]), L.dptr(keep[6]))
        self._create((_di_params(scen.params), w, self.dims, init, _di_opts(tol, max_iter, fp32)), log, log_separation)

    def step(self, rounds=1):
        """Runs ``rounds`` rounds (one host synchronisation, at the end); returns the number done."""
        done = ct.c_int()
        self._call("step", int(rounds), ct.byref(done))
        return done.value

    def read(self):
        """The latest round: dict of z, kkt, iters, status, x0, u_prev (the next round's), nbr."""
        r = dict(z=np.zeros((self.B, self.nz)), kkt=np.zeros(self.B), iters=np.zeros(self.B, np.int32),
                 status=np.zeros(self.B, np.int32), x0=np.zeros((self.B, self.nx)), u_prev=np.zeros((self.B, self.nu)),
                 nbr=np.zeros((self.B, self.nb), np.int32))
        o = L.cmpc_di_rounds_out(L.dptr(r["z"]), L.dptr(r["kkt"]), L.iptr(r["iters"]), L.iptr(r["status"]),
                                 L.dptr(r["x0"]), L.dptr(r["u_prev"]), L.iptr(r["nbr"]) if self.nb else None)
        self._call("read", ct.byref(o))
        return r

    def history(self, first, count):
        """kkt, iters, status of rounds [first, first + count) (counted from create), each (count, B); a round
        not yet run or already overwritten raises CmpcError(CMPC_ERR_ARG)."""
        count = int(count)
        r = dict(kkt=np.zeros((max(count, 0), self.B)), iters=np.zeros((max(count, 0), self.B), np.int32),
                 status=np.zeros((max(count, 0), self.B), np.int32))
        self._call("history", int(first), count, L.dptr(r["kkt"]), L.iptr(r["iters"]), L.iptr(r["status"]))
        return r


class LinRoundsHandle(_RoundsHandle):
    """Consensus rounds of agents with any linear model through the C ABI's round handle (cmpc_lin_rounds_*): the
    library owns the device state; no torch.  ``shared``: dims and weights (nx, nu, N, ns, mc = mo + nb, Q, R, dR,
    Qs, u_ub, u_lb, row_slack, row_sign); ``prm``: dict(ix, iy, min_dist, wq); ``own``: dict(qlin_own, C_own,
    h_own) (``scenarios.lin_rows``); population arrays A (n, N, nx, nx), B (n, N, nx, nu), x0 (n, nx), u_prev
    (n, nu), nbr (n, nb), own arrays with leading dimension n, traj (n, N+1, 2): this handle takes the contiguous
    shard ``rank`` of ``world``.  A ``prm`` with ``iz`` makes the positions 3-D (cmpc_lin_rounds_create3): traj and
    ``get_traj`` / ``set_traj`` are x 3, and re-selection and the log's separation use the 3-D distance.
    ``opts``: a ``_lib.opts`` for the solver (None: defaults).  ``host_exchange``, ``reselect``, ``lpt``,
    ``history``, ``log``, ``log_separation``: as ``DIRoundsHandle`` (``lpt`` None: its default rule).
    ``set_state`` replaces the predicted state by a measured one."""

    _fn = "cmpc_lin_rounds_"

    def _shard(self, shared, prm, traj, x0, nbr, rank, world, ctx, opts, host_exchange, reselect, lpt, history):
        """The wrapper's attributes and cmpc_lin_rounds_dims; returns (this rank's slice, nbr as (n, nb) int32)."""
        n = int(np.shape(x0)[0])
        if n % world:
            raise ValueError("agents must be divisible by the number of ranks")
        self.pd = _pos_dim(prm)
        if np.shape(traj) != (n, int(shared["N"]) + 1, self.pd):
            raise ValueError(f"traj: (n, N+1, {self.pd})")
        self.ctx = ctx or L.default_context(0)
        self.B, self.n, self.N = n // world, n, int(shared["N"])
        sl = slice(rank * self.B, (rank + 1) * self.B)
        nbr = L.i32(np.asarray(nbr).reshape(n, -1))
        self.nb, self.nx, self.nu, self.ns = nbr.shape[1], int(shared["nx"]), int(shared["nu"]), int(shared["ns"])
        self.mo = int(shared["mc"]) - self.nb
        self.nz = nz_of(shared)
        fp32 = bool(opts is not None and opts.flags & L.CMPC_FLAG_FP32)
        self.lpt = _lpt_default(shared, self.N, fp32) if lpt is None else bool(lpt)
        flags = self._flags(host_exchange, reselect=reselect, lpt=self.lpt)
        self.dims = L.cmpc_lin_rounds_dims(n, self.B, sl.start, self.N, self.nb, flags, int(history), self.nx, self.nu,
                                           self.ns, self.mo)
        return sl, nbr

    def __init__(self, shared, prm, own, A, B, x0, u_prev, nbr, traj, rank=0, world=1, ctx=None, opts=None,
                 host_exchange=False, reselect=False, lpt=None, history=1, log=0, log_separation=False):
        sl, nbr = self._shard(shared, prm, traj, x0, nbr, rank, world, ctx, opts, host_exchange, reselect, lpt,
                              history)
        w, wkeep = _weights(shared)
        opt = lambda a: None if a is None or self.mo == 0 else L.f64(np.asarray(a)[sl])   # noqa: E731
        keep = [L.f64(np.asarray(A)[sl]), L.f64(np.asarray(B)[sl]), L.f64(np.asarray(x0)[sl]),
                L.f64(np.asarray(u_prev)[sl]), L.f64(np.asarray(own["qlin_own"])[sl]), opt(own.get("C_own")),
                opt(own.get("h_own")), L.i32(nbr[sl]), L.f64(traj)]
        init = L.cmpc_lin_rounds_init(*[L.dptr(a) for a in keep[:7]], L.iptr(keep[7]) if self.nb else None,
                                      L.dptr(keep[8]))
        self._create((_lin_params(prm), w, self.dims, init, opts if opts is not None else L.opts()), log,
                     log_separation, create="create3" if self.pd == 3 else "create")

    @classmethod
    def of_di(cls, scen, tol=None, max_iter=None, fp32=False, **kw):
        """The handle of a ``scenarios.DIScenario`` expressed in this family (``scenarios.lin_of_di``): round for
        round what ``DIRounds(scen, fused=False)`` computes."""
        from .scenarios import lin_of_di

        lin = lin_of_di(scen)
        return cls(scen.shared, lin["prm"], lin["own"], scen.A, scen.B, scen.x0, scen.u_prev, scen.nbr, scen.traj,
                   opts=_di_opts(tol, max_iter, fp32), **kw)

    @classmethod
    def of_di3(cls, scen, alt, tol=None, max_iter=None, fp32=False, **kw):
        """The handle of a 3-D ``scenarios.DIScenario`` with 3-D positions (``scenarios.lin3_of_di``): the agents at
        altitude ``alt`` (a scalar or (n,)), the altitude in the collision planes, the coverage term and the
        neighbour selection.  With ``alt`` one value the first round is ``of_di``'s."""
        from .scenarios import lin3_of_di

        lin = lin3_of_di(scen, alt)
        return cls(scen.shared, lin["prm"], lin["own"], scen.A, scen.B, lin["x0"], scen.u_prev, scen.nbr, lin["traj"],
                   opts=_di_opts(tol, max_iter, fp32), **kw)

    @property
    def pos_dim(self):
        """Coordinates of a position on this handle (cmpc_lin_rounds_pos_dim): 2, or 3 when ``prm`` has ``iz``."""
        pd = ct.c_int()
        self._call("pos_dim", ct.byref(pd))
        return pd.value

    def step(self, rounds=1):
        """Runs ``rounds`` rounds (one host synchronisation, at the end); returns the number done."""
        done = ct.c_int()
        self._call("step", int(rounds), ct.byref(done))
        return done.value

    def step_consensus(self, steps=1, min_rounds=3, need=2, max_rounds=12, atol=0.01, rtol=1e-5):
        """Runs ``steps`` consensus steps (cmpc_lin_rounds_step_consensus): each repeats build, solve, publish and
        exchange at the handle's state (and table time) until the published positions agree — the rule of
        ``scenarios.consensus_stop`` on the node-wide counts of ``scenarios.lin_publish`` — and then advances.  A
        consensus step is one round for ``history``, ``log`` and ``time``; ``max_rounds=1`` is ``step(1)``.  The
        defaults are the reference's loop (NL_EU_N_main.py:102-162).  Returns (steps done, inner rounds run)."""
        co = L.cmpc_consensus_opts(int(min_rounds), int(need), int(max_rounds), float(atol), float(rtol))
        done, inner = ct.c_int(), ct.c_int()
        self._call("step_consensus", int(steps), ct.byref(co), ct.byref(done), ct.byref(inner))
        return done.value, inner.value

    def read(self):
        """The latest round: dict of z, kkt, iters, status, x0, u_prev (the next round's), nbr."""
        r = dict(z=np.zeros((self.B, self.nz)), kkt=np.zeros(self.B), iters=np.zeros(self.B, np.int32),
                 status=np.zeros(self.B, np.int32), x0=np.zeros((self.B, self.nx)), u_prev=np.zeros((self.B, self.nu)),
                 nbr=np.zeros((self.B, self.nb), np.int32))
        o = L.cmpc_lin_rounds_out(L.dptr(r["z"]), L.dptr(r["kkt"]), L.iptr(r["iters"]), L.iptr(r["status"]),
                                  L.dptr(r["x0"]), L.dptr(r["u_prev"]), L.iptr(r["nbr"]) if self.nb else None)
        self._call("read", ct.byref(o))
        return r

    def history(self, first, count):
        """kkt, iters, status of rounds [first, first + count) (counted from create), each (count, B); a round
        not yet run or already overwritten raises CmpcError(CMPC_ERR_ARG)."""
        count = int(count)
        r = dict(kkt=np.zeros((max(count, 0), self.B)), iters=np.zeros((max(count, 0), self.B), np.int32),
                 status=np.zeros((max(count, 0), self.B), np.int32))
        self._call("history", int(first), count, L.dptr(r["kkt"]), L.iptr(r["iters"]), L.iptr(r["status"]))
        return r

    def set_state(self, x0=None, u_prev=None):
        """The next round solves from ``x0`` (B, nx) and ``u_prev`` (B, nu) instead of the predicted ones (None:
        that part stays): the measured state of a real loop."""
        a = None if x0 is None else L.f64(x0)
        b = None if u_prev is None else L.f64(u_prev)
        if (a is not None and a.shape != (self.B, self.nx)) or (b is not None and b.shape != (self.B, self.nu)):
            raise ValueError("x0: (B, nx), u_prev: (B, nu)")
        self._call("set_state", L.dptr(a), L.dptr(b))


class LinTableRoundsHandle(LinRoundsHandle):
    """``LinRoundsHandle`` for time-varying agents (cmpc_lin_rounds_create_table): the model, the own cost and the
    own rows are a stage table, and round r plans with the table's window at the handle's time — stages t .. t+N,
    ``scenarios.lin_window`` — which a round that ran moves on one stage.  ``table``: dict of population arrays
    A (n, T, nx, nx), B (n, T, nx, nu), qlin (n, T, nx), C (n, T, mo, nx), h (n, T, mo) (C / h None when the agents
    have no own rows); ``mode``: ``CMPC_TABLE_HOLD`` (past its end the table holds its last stage) or
    ``CMPC_TABLE_PERIODIC``; ``t0``: the first round's time.  Everything else as ``LinRoundsHandle``."""

    def __init__(self, shared, prm, table, x0, u_prev, nbr, traj, mode=L.CMPC_TABLE_HOLD, t0=0, rank=0, world=1,
                 ctx=None, opts=None, host_exchange=False, reselect=False, lpt=None, history=1, log=0,
                 log_separation=False):
        from .scenarios import lin_table_rows_of

        self.T, self.mode = lin_table_rows_of(table), int(mode)
        sl, nbr = self._shard(shared, prm, traj, x0, nbr, rank, world, ctx, opts, host_exchange, reselect, lpt,
                              history)
        w, wkeep = _weights(shared)
        opt = lambda a: None if a is None or self.mo == 0 else L.f64(np.asarray(a)[sl])   # noqa: E731
        keep = [L.f64(np.asarray(table[k])[sl]) for k in ("A", "B", "qlin")] + \
            [opt(table.get("C")), opt(table.get("h")), L.f64(np.asarray(x0)[sl]), L.f64(np.asarray(u_prev)[sl])]
        knbr, ktraj = L.i32(nbr[sl]), L.f64(traj)
        init = L.cmpc_lin_rounds_table_init(self.T, self.mode, int(t0), *[L.dptr(a) for a in keep],
                                            L.iptr(knbr) if self.nb else None, L.dptr(ktraj))
        self._create((_lin_params(prm), w, self.dims, init, opts if opts is not None else L.opts()), log,
                     log_separation, create="create_table3" if self.pd == 3 else "create_table")

    @classmethod
    def of_di(cls, scen, tol=None, max_iter=None, fp32=False, T=1, **kw):
        """The handle of a ``scenarios.DIScenario`` as a stage table of ``T`` equal rows under CMPC_TABLE_HOLD
        (``scenarios.lin_table_of_di``): round for round what ``LinRoundsHandle.of_di(scen)`` computes."""
        from .scenarios import lin_table_of_di

        lin = lin_table_of_di(scen, T)
        return cls(scen.shared, lin["prm"], lin["table"], scen.x0, scen.u_prev, scen.nbr, scen.traj, mode=lin["mode"],
                   opts=_di_opts(tol, max_iter, fp32), **kw)

    @classmethod
    def of_di3(cls, scen, alt, tol=None, max_iter=None, fp32=False, T=1, **kw):
        """``LinRoundsHandle.of_di3`` as a stage table of ``T`` equal rows under CMPC_TABLE_HOLD."""
        from .scenarios import lin3_of_di, lin_table_of_di

        lin, tab = lin3_of_di(scen, alt), lin_table_of_di(scen, T)
        return cls(scen.shared, lin["prm"], tab["table"], lin["x0"], scen.u_prev, scen.nbr, lin["traj"], mode=tab["mode"],
                   opts=_di_opts(tol, max_iter, fp32), **kw)

    @property
    def time(self):
        """The time t of the next round: it plans with table rows row(t) .. row(t + N)."""
        t = ct.c_int()
        self._call("get_time", ct.byref(t))
        return t.value

    def set_time(self, t):
        """The next round plans at time ``t`` (0 <= t < T)."""
        self._call("set_time", int(t))

    def write_table(self, first_row, A=None, B=None, qlin=None, C=None, h=None):
        """Overwrites table rows [first_row, first_row + count) of this handle's agents: each array given is (B,
        count, ...) in the table's shapes with ``count`` for T (the same count in every one); None: that part stays
        as it was.  No wrap: split a write that passes the table's end.  Carrying A or B withdraws CMPC_FLAG_LTI."""
        nx, nu, mo = self.nx, self.nu, self.mo
        tail = dict(A=(nx, nx), B=(nx, nu), qlin=(nx,), C=(mo, nx), h=(mo,))
        arrs = {k: L.f64(v) for k, v in dict(A=A, B=B, qlin=qlin, C=C, h=h).items() if v is not None}
        counts = {a.shape[1] for a in arrs.values() if a.ndim >= 2}
        if len(counts) > 1 or any(a.ndim < 2 or a.shape != (self.B, a.shape[1]) + tail[k] for k, a in arrs.items()):
            raise ValueError("write_table: arrays (B, count, ...) in the table's shapes, one count")
        if mo == 0:                                         # (no own rows: nothing to hand over)
            arrs.pop("C", None), arrs.pop("h", None)
        rows = L.cmpc_lin_table(*[L.dptr(arrs.get(k)) for k in ("A", "B", "qlin", "C", "h")])
        self._call("table_write", int(first_row), counts.pop() if counts else 0, ct.byref(rows))
