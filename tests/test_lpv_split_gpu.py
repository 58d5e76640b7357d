"""CMPC_FLAG_LPV_SPLIT on the GPU (include/cmpc.h): the partition kernel (csrc/mpc_lpv_split.hip) against its numpy
statement, and a mixed batch whose agents each come back bit for bit as their reference call returns them - a
conforming agent as under the promise (CMPC_FLAG_LPV, the compact instantiation), any other as with no structure
flag (the general one) - on the host entries, the device entries, with duals, with the certificate, and through the
osqp_solve_qp adapter.

The planted violations are those of lpv_level_cases.PLANTS but the NaN: a NaN agent's solve says nothing about the
routing, and the detector's own test covers its level."""

import numpy as np
import pytest

from conftest import KKT_TOL, assert_matches_optimum
from lpv_level_cases import PER_AGENT, PLANTS, copy_of, osqp_args, plant, recognised, stacked, tiled
from test_lpv_level_gpu import COMP_REL, _di_batch

pytestmark = pytest.mark.gpu

OUT = ("z", "kkt", "iters", "status")
DUAL_OUT = OUT + ("y", "dua_res")
SPLIT, LPV, AUTO = 65536, 16384, 32768
SENTINEL = -7


# ---------------------------------------------------------------- the partition kernel
def _patterns(batch, rng):
    first = np.zeros(batch, np.int32)
    first[0] = 2
    last = np.zeros(batch, np.int32)
    last[-1] = 1
    return {"all 0": np.zeros(batch, np.int32), "all 2": np.full(batch, 2, np.int32),
            "alternating": (np.arange(batch) % 2).astype(np.int32) * 2, "first": first, "last": last,
            "random": rng.integers(0, 3, batch).astype(np.int32)}


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_partition_matches_the_numpy_statement(gpu_ctx, batch):
    from cmpc import structure as St

    rng = np.random.default_rng(100 + batch)
    for tag, level in _patterns(batch, rng).items():
        conf, rest = St.lpv_split_gpu(level, gpu_ctx, fill=SENTINEL)
        wc, wr = St.lpv_split(level)
        # the statement marks the entries the kernel leaves alone with -1: there the sentinel must have stayed
        np.testing.assert_array_equal(conf, np.where(wc == -1, SENTINEL, wc), err_msg=f"{batch} {tag}: conf")
        np.testing.assert_array_equal(rest, np.where(wr == -1, SENTINEL, wr), err_msg=f"{batch} {tag}: rest")
        assert conf[batch] + rest[batch] == batch and conf[batch] == (level > 0).sum()


def test_partition_arguments(gpu_ctx):
    import torch

    from cmpc import _lib as L
    from cmpc import structure as St
    from cmpc.solver import _tptr

    dev = torch.device("cuda", gpu_ctx.device)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    batch = 6
    level = torch.tensor([2, 0, 0, 1, 2, 0], dtype=torch.int32, device=dev)
    buf = torch.full((3 * (batch + 1),), SENTINEL, dtype=torch.int32, device=dev)
    conf, rest = buf[:batch + 1], buf[batch + 1:2 * (batch + 1)]

    def call(n, lv, a, b):
        return lib.cmpc_mpc_lpv_split_dev(h, n, lv, a, b, None)

    lv, pc, pr = _tptr(level), _tptr(conf), _tptr(rest)
    assert call(0, None, None, None) == L.CMPC_OK                # batch 0: no launch, nothing read or written
    assert call(0, lv, pc, pr) == L.CMPC_OK
    assert call(-1, lv, pc, pr) == L.CMPC_ERR_ARG
    assert call(batch, None, pc, pr) == L.CMPC_ERR_ARG
    assert call(batch, lv, None, pr) == L.CMPC_ERR_ARG
    assert call(batch, lv, pc, None) == L.CMPC_ERR_ARG
    assert call(batch, lv, pc, pc) == L.CMPC_ERR_ARG             # conf is rest
    assert call(batch, lv, pc, _tptr(buf[batch:])) == L.CMPC_ERR_ARG      # ... or shares its last int with it
    assert call(batch, pc, pc, pr) == L.CMPC_ERR_ARG             # level is conf
    assert call(batch, _tptr(buf[1:]), pc, pr) == L.CMPC_ERR_ARG          # ... or lies inside it
    assert call(batch, _tptr(buf[batch + 2:]), pc, pr) == L.CMPC_ERR_ARG  # level inside rest
    torch.cuda.synchronize(dev)
    assert (buf.cpu().numpy() == SENTINEL).all()                 # none of these wrote anything
    # adjacent buffers do not alias: the call goes through and is right
    assert call(batch, lv, pc, pr) == L.CMPC_OK
    torch.cuda.synchronize(dev)
    wc, wr = St.lpv_split(level.cpu().numpy())
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[:batch + 1], np.where(wc == -1, SENTINEL, wc))
    np.testing.assert_array_equal(got[batch + 1:2 * (batch + 1)], np.where(wr == -1, SENTINEL, wr))
    assert (got[2 * (batch + 1):] == SENTINEL).all()


# ---------------------------------------------------------------- mixed batches
def _solve(p, ctx, duals=False, **kw):
    from cmpc.solver import solve_mpc

    kw.setdefault("rescue", True)
    kw.setdefault("polish", True)
    return dict(zip(DUAL_OUT if duals else OUT, solve_mpc(p, ctx, duals=duals, **kw)))


def _same(a, b, tag):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k}")


def _routed(split, promise, plain, conforming, tag):
    """Per agent: the promise's rows where the agent conforms, the plain call's elsewhere."""
    for k in split:
        want = np.where(conforming.reshape((-1,) + (1,) * (promise[k].ndim - 1)), promise[k], plain[k])
        np.testing.assert_array_equal(split[k], want, err_msg=f"{tag}: {k}")


def _mixed_batch(name, batch, seed):
    """The captured agents tiled to `batch`, violations planted in about a third of them (three at least): agent 0,
    the last agent and a seeded choice of the others with one of PLANTS each, and agent 1 with the plant of
    test_lpv_level_gpu._break_promise (B's row 3 at every stage), which moves that agent by more than 1e-3 - a
    single entry at a single stage need not (measured: agent 0 of lpv_n10_a2 moves by 2e-12 under that very plant)."""
    p = stacked(name)
    if batch != p["A"].shape[0]:
        p = tiled(p, batch)
    N, mc = int(p["N"]), int(p["mc"])
    rng = np.random.default_rng(seed)
    want = max(3, round(batch / 3))
    others = rng.choice(np.arange(2, batch - 1), size=want - 3, replace=False)
    agents = sorted({0, 1, batch - 1} | set(int(a) for a in others))
    kinds = [w for w, (nm, idx, val) in enumerate(PLANTS)
             if not (isinstance(val, float) and np.isnan(val)) and not (nm == "C" and idx[0] >= mc)]
    for n, a in enumerate(agents):
        if a == 1:
            p["B"][1, :, 3, 0] = 0.5
        else:
            plant(p, a, kinds[n % len(kinds)], (0, N - 1, N // 2)[n % 3])
    return p, np.array(agents)


_MIXED = {}


def _mixed(ctx, name, batch):
    """(batch dict, planted agents, promise, plain, split) of one mixed batch: solved once, shared, read-only."""
    key = (name, batch)
    if key not in _MIXED:
        p, agents = _mixed_batch(name, batch, seed=batch)
        _MIXED[key] = (p, agents, _solve(p, ctx, lpv=True), _solve(p, ctx), _solve(p, ctx, lpv="split"))
    return _MIXED[key]


# Planted: about a third of the agents, but never fewer than three (_mixed_batch): agent 0, the last agent, and agent
# 1, whose plant is not one of PLANTS but _break_promise's (B's row 3 at every stage), the only one known to move its
# agent by more than 1e-3.  So the 5-agent case plants agents 0, 1 and 4, three of five; 70 agents: 23; 12 agents: 4.
@pytest.mark.parametrize("name,batch", [("lpv_n10_a2", 5), ("lpv_n10_a2", 70), ("lpv_n30_a3", 12)])
def test_mixed_batch_is_routed_per_agent(gpu_ctx, name, batch):
    from cmpc import structure as St

    p, agents, promise, plain, split = _mixed(gpu_ctx, name, batch)
    assert p["A"].shape[0] == batch and agents[0] == 0 and agents[-1] == batch - 1
    level = St.lpv_level(p)
    conforming = level > 0
    assert sorted(np.nonzero(~conforming)[0].tolist()) == agents.tolist()
    assert np.array_equal(St.lpv_level_gpu(p, gpu_ctx), level)
    dz = np.abs(plain["z"] - promise["z"]).max(axis=1)
    print(f"{name} x{batch}: {agents.size} planted {agents.tolist()}; max|z_plain - z_promise| over the planted "
          f"{dz[agents].max():.3e} (agent 1: {dz[1]:.3e}), over the others {dz[conforming].max():.2e}; "
          f"statuses of the planted {split['status'][agents].tolist()}")
    _routed(split, promise, plain, conforming, f"{name} x{batch}")
    assert (split["status"][conforming] == 1).all(), split["status"]
    # the general kernel really ran: some planted agent is not where the compact kernel puts it
    assert np.abs(split["z"] - promise["z"])[agents].max() > 1e-3, dz[agents]


def _device_batch(p, dev):
    import torch

    return {k: torch.as_tensor(np.ascontiguousarray(p[k], dtype=np.float64), device=dev) for k in PER_AGENT}


def _device_out(p, dev, duals=False):
    import torch

    from cmpc.duals import ny_of
    from cmpc.solver import nz_of

    batch = p["A"].shape[0]
    out = dict(z=torch.zeros((batch, nz_of(p)), dtype=torch.float64, device=dev),
               kkt=torch.zeros(batch, dtype=torch.float64, device=dev),
               iters=torch.zeros(batch, dtype=torch.int32, device=dev),
               status=torch.zeros(batch, dtype=torch.int32, device=dev))
    if duals:
        out["y"] = torch.zeros((batch, ny_of(p)), dtype=torch.float64, device=dev)
        out["dua_res"] = torch.zeros(batch, dtype=torch.float64, device=dev)
    return out


def test_device_entry_decides_on_every_call(gpu_ctx):
    import torch

    from cmpc import _lib as L
    from cmpc.solver import solve_mpc_dev

    p, agents, _, _, split = _mixed(gpu_ctx, "lpv_n10_a2", 70)
    dev = torch.device("cuda", gpu_ctx.device)
    t = _device_batch(p, dev)
    rp = L.CMPC_FLAG_RESCUE | L.CMPC_FLAG_POLISH
    out = _device_out(p, dev)
    solve_mpc_dev(p, t, out, gpu_ctx, lpv="split", flags=rp)
    torch.cuda.synchronize(dev)
    _same(split, {k: out[k].cpu().numpy() for k in OUT}, "device entry, rescue and polish")
    # without rescue the solve needs no scratch of its own: the lists still get theirs
    out = _device_out(p, dev)
    solve_mpc_dev(p, t, out, gpu_ctx, lpv="split")
    torch.cuda.synchronize(dev)
    bare = _solve(p, gpu_ctx, lpv="split", rescue=False, polish=False)
    _same(bare, {k: out[k].cpu().numpy() for k in OUT}, "device entry, no rescue")
    _routed(bare, _solve(p, gpu_ctx, lpv=True, rescue=False, polish=False),
            _solve(p, gpu_ctx, rescue=False, polish=False), ~np.isin(np.arange(70), agents), "no rescue")
    # a new pattern in the device tensors: agent 1 restored, a conforming copy of it planted instead; nothing else
    # is uploaded
    captured = stacked("lpv_n10_a2")
    ncap = captured["A"].shape[0]
    fresh = next(a for a in range(2, 70) if a not in agents and a % ncap == 1)
    q = copy_of(p)
    q["B"][1] = captured["B"][1]
    q["B"][fresh, :, 3, 0] = 0.5
    t["B"][1] = torch.as_tensor(q["B"][1], device=dev)
    t["B"][fresh, :, 3, 0] = 0.5
    out = _device_out(p, dev)
    solve_mpc_dev(p, t, out, gpu_ctx, lpv="split", flags=rp)
    torch.cuda.synchronize(dev)
    got = {k: out[k].cpu().numpy() for k in OUT}
    want = _solve(q, gpu_ctx, lpv="split")
    _same(want, got, "device entry, second pattern")
    assert np.abs(got["z"][1] - split["z"][1]).max() > 1e-3 and np.abs(got["z"][fresh] - split["z"][fresh]).max() > 1e-3
    promise = _solve(q, gpu_ctx, lpv=True)
    np.testing.assert_array_equal(got["z"][1], promise["z"][1])
    assert np.abs(got["z"][fresh] - promise["z"][fresh]).max() > 1e-3
    # CMPC_FLAG_LPV_AUTO keeps its rule here, alone and with the new flag
    for kw in (dict(lpv="auto"), dict(lpv="auto", flags=SPLIT)):
        with pytest.raises(L.CmpcError) as e:
            solve_mpc_dev(p, t, out, gpu_ctx, **kw)
        assert e.value.code == L.CMPC_ERR_ARG


def test_all_or_none_conforming_and_flag_precedence(gpu_ctx):
    p = stacked("lpv_n10_a2")
    promise = _solve(p, gpu_ctx, lpv=True)
    _same(promise, _solve(p, gpu_ctx, lpv="split"), "all conforming: the promise")
    q = copy_of(p)
    q["B"][:, :, 3, 0] = 0.5
    _same(_solve(q, gpu_ctx), _solve(q, gpu_ctx, lpv="split"), "none conforming: the plain call")
    # with CMPC_FLAG_LPV the promise wins: nothing is detected, the planted entries are not read
    m, _, mp, _, ms = _mixed(gpu_ctx, "lpv_n10_a2", 5)
    _same(mp, _solve(m, gpu_ctx, flags=SPLIT | LPV), "split | promise")
    _same(mp, _solve(m, gpu_ctx, flags=SPLIT | LPV | AUTO), "all three")
    # with CMPC_FLAG_LPV_AUTO on a host entry the split decides (auto alone would run the general kernel everywhere)
    _same(ms, _solve(m, gpu_ctx, flags=SPLIT | AUTO), "split | auto")


def test_duals_are_routed_too(gpu_ctx):
    from cmpc import _lib as L
    from cmpc import structure as St
    from cmpc.solver import solve_mpc_dev

    p, agents, promise, plain, split = _mixed(gpu_ctx, "lpv_n10_a2", 5)
    conforming = St.lpv_level(p) > 0
    dp, dn, ds = (_solve(p, gpu_ctx, duals=True, **kw) for kw in (dict(lpv=True), dict(), dict(lpv="split")))
    _routed(ds, dp, dn, conforming, "duals")
    _same(split, {k: ds[k] for k in OUT}, "duals move nothing")
    assert np.isfinite(ds["y"][conforming]).all() and (ds["status"][conforming] == 1).all()
    assert not np.array_equal(dp["y"][1], dn["y"][1])
    # ... and on the device entry
    import torch

    dev = torch.device("cuda", gpu_ctx.device)
    out = _device_out(p, dev, duals=True)
    solve_mpc_dev(p, _device_batch(p, dev), out, gpu_ctx, lpv="split", flags=L.CMPC_FLAG_RESCUE | L.CMPC_FLAG_POLISH)
    torch.cuda.synchronize(dev)
    _same(ds, {k: out[k].cpu().numpy() for k in DUAL_OUT}, "duals, device entry")


def test_certificate_follows_on_the_whole_batch(gpu_ctx):
    from cmpc import structure as St

    p, agents, _, _, _ = _mixed(gpu_ctx, "lpv_n10_a2", 5)
    q = copy_of(p)
    hard = next(a for a in range(5) if a not in agents)
    q["h"][hard, :, 0] = -50.0          # the minimum-speed row out of reach (tests/test_infeas_gpu.py): hard-infeasible
    conforming = St.lpv_level(q) > 0
    assert conforming[hard] and not conforming[agents].any()
    kw = dict(certify=True, max_iter=40)
    promise, plain, split = _solve(q, gpu_ctx, lpv=True, **kw), _solve(q, gpu_ctx, **kw), _solve(q, gpu_ctx, lpv="split", **kw)
    _routed(split, promise, plain, conforming, "certify")
    assert split["status"][hard] == -3, split["status"]
    assert _solve(q, gpu_ctx, lpv="split", max_iter=40)["status"][hard] not in (1, 2, -3)


@pytest.mark.parametrize("case", ["di", "n125", "generic"])
def test_flag_is_ignored_where_the_batch_is_not_eligible(gpu_ctx, case):
    from cmpc.solver import plan

    kw = {}
    if case == "di":
        p = _di_batch()
    elif case == "n125":
        p = stacked("lpv_n125_a3")
        for k in PER_AGENT:
            p[k] = np.ascontiguousarray(p[k][:2])
    else:
        p = stacked("lpv_n10_a2")
        kw = dict(generic=True)
    batch = p["A"].shape[0]
    base = _solve(p, gpu_ctx, **kw)
    info = plan(p, batch, rescue=True, polish=True, **kw)
    assert info["solver"] == {"di": "condensed_v3", "n125": "riccati", "generic": "condensed"}[case]
    _same(base, _solve(p, gpu_ctx, lpv="split", **kw), f"{case} lpv='split'")
    _same(base, _solve(p, gpu_ctx, flags=SPLIT | AUTO, **kw), f"{case} split | auto")
    assert plan(p, batch, rescue=True, polish=True, flags=SPLIT, **kw) == info


def test_adapter_routes_one_qp_off_the_pattern(gpu_ctx):
    """The 12 captured lpv_n30_a3 QPs through osqp_solve_qp_batch(lpv_structure="split") with QP 1 moved off the
    pattern (B's row 3, still a reference-form QP): the untouched QPs meet the bars of
    test_routed_adapter_on_the_captured_qps and are what the all-conforming routed call returns; the moved one meets
    the same bars on its own data (its optimum from oracle.qp_ipm) and is what the default adapter returns."""
    import cmpc
    from cmpc import structure as St
    from oracle import qp_ipm

    rec = recognised("lpv_n30_a3")
    assert len(rec) == 12
    qps = [osqp_args(c) for c, _ in rec]
    moved = copy_of(rec[1][1])
    moved["B"][0, :, 3, 0] = 0.5
    qps[1] = St.reference_form(moved, 0)
    back = St.recognize(*qps[1])
    assert back is not None and St.lpv_level(back)[0] == 0 and St.shared_key(back) == St.shared_key(rec[0][1])
    out = cmpc.osqp_solve_qp_batch(qps, ctx=gpu_ctx, lpv_structure="split")
    routed = cmpc.osqp_solve_qp_batch([osqp_args(c) for c, _ in rec], ctx=gpu_ctx, lpv_structure=True)
    default = cmpc.osqp_solve_qp_batch(qps, ctx=gpu_ctx)
    # the moved QP in the captured QPs' form, from its own data: A = [G; Aeq] (the order of res.y), its optimum from
    # the dense reference solver
    P1, q1, G1, h1, A1, b1 = qps[1]
    Aall = np.vstack([G1.toarray(), A1.toarray()])
    c1 = dict(P=P1.toarray(), q=np.asarray(q1, float), A=Aall, l=np.concatenate([np.full(h1.size, -np.inf), b1]),
              u=np.concatenate([h1, b1]))
    ref = qp_ipm.solve_qp(c1["P"], c1["q"], c1["A"], c1["l"], c1["u"])
    assert ref.status == "solved", ref.status
    c1["z"], c1["y"] = ref.x, ref.y
    cases = [c for c, _ in rec]
    cases[1] = c1
    for j, (c, (res, feasible)) in enumerate(zip(cases, out)):
        assert res.info.solver == "structured"
        cert = qp_ipm.kkt_certificate(c["P"], c["q"], c["A"], c["l"], c["u"], res.x, res.y)
        ys = max(1.0, np.abs(res.y).max())
        if j == 1:
            print(f"moved QP: status {res.info.status_val} iters {res.info.iter} kkt {res.info.kkt:.2e} pri_res "
                  f"{res.info.pri_res:.2e} max|x - x*| {np.abs(res.x - c['z']).max():.2e} stat_rel {cert['stat_rel']:.2e} "
                  f"prim {cert['prim']:.2e} comp/|y| {cert['comp'] / ys:.2e} sign {cert['dual_sign']:.1e}; "
                  f"max|x - x_routed| {np.abs(res.x - routed[1][0].x).max():.2e}")
        # the bars of test_routed_adapter_on_the_captured_qps, on every QP, the moved one included
        assert feasible == 1 and res.info.status_val == 1, (j, res.info.status)
        assert res.info.kkt <= 1e-6 and res.info.pri_res <= 1e-6, (j, res.info.kkt, res.info.pri_res)
        assert_matches_optimum(res.x, c, 1e-6)
        assert res.y is not None and res.y.shape == c["y"].shape and np.isfinite(res.y).all()
        assert cert["stat_rel"] <= KKT_TOL and cert["prim"] <= KKT_TOL, (j, cert)
        assert cert["dual_sign"] == 0.0, (j, cert)
        assert cert["comp"] <= COMP_REL * ys, (j, cert)
        # an untouched QP is what the all-conforming routed call returns, the moved one what the default adapter does
        want = default[1][0] if j == 1 else routed[j][0]
        assert np.array_equal(res.x, want.x) and np.array_equal(res.y, want.y)
        assert res.info.status_val == want.info.status_val and res.info.iter == want.info.iter
    # the general kernel really solved the moved QP: the compact one, blind to the moved entries, lands elsewhere
    assert np.abs(out[1][0].x - routed[1][0].x).max() > 1e-3
