"""The combined-row infeasibility certificate on the GPU (csrc/mpc_infeas_rows.hip; CMPC_FLAG_CERTIFY_ROWS,
cmpc_mpc_certify_rows): the kernel against its numpy statement (cmpc.infeas.certify_rows) and the reference-form
matrices, the device entry point against the host one, the solves with certify="rows" against the same solves
with certify=True and without, and the osqp_solve_qp drop-in."""
import ctypes as ct

import numpy as np
import pytest

from conftest import lpv_qps
from test_infeas_gpu import _di_with_an_infeasible_and_a_nan_agent, _osqp_args
from test_infeas_rows_host import ALL, check_rows_ray, plant_consecutive, reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", ALL)
def test_kernel_matches_the_numpy_statement_and_the_ray_verifies(gpu_ctx, i):
    """Status, iters and nrows equal; ray and margin within 1e-10 of the statement, relative to max(1, |y|inf) as
    in tests/test_infeas_gpu.py.  Measured on one MI355X: 2.4e-13 at most (the margin alone, relative to itself,
    2.0e-11); the CPU statement's own sensitivity to the order of summation is 1.7e-13
    (tests/test_infeas_rows_host.py), so the bar leaves more than two orders of magnitude.  No seed lands within
    1e-6 relative of the threshold at its certifying check (asserted in the host test)."""
    from cmpc import infeas

    p, ks, single, ref = reference(i)
    assert (single["row"] == -1).all()            # ground the single-row rule does not cover
    got = infeas.certify_rows_gpu(p, ctx=gpu_ctx)
    print(f"shape {i}: iters {got['iters']} (numpy {ref['iters']}) nrows {got['nrows']}")
    assert np.array_equal(got["status"], ref["status"]) and (got["status"] == -3).all()
    assert np.array_equal(got["iters"], ref["iters"]), (got["iters"], ref["iters"])
    assert np.array_equal(got["nrows"], ref["nrows"])
    dev = rel = 0.0
    for a in range(p["A"].shape[0]):
        y = got["ray"][a]
        scale = max(1.0, np.abs(ref["ray"][a]).max())   # (the measure of tests/test_infeas_gpu.py)
        dev = max(dev, np.abs(y - ref["ray"][a]).max() / scale, abs(got["margin"][a] - ref["margin"][a]) / scale)
        rel = max(rel, abs(got["margin"][a] - ref["margin"][a]) / abs(ref["margin"][a]))
        res, gap = check_rows_ray(p, a, y)
        print(f"shape {i} agent {a}: margin {got['margin'][a]:.3e} residual {res:.2e} gap {gap:.6f} "
              f"|y|inf {np.abs(y).max():.2e}")
    print(f"shape {i}: max deviation from the numpy statement {dev:.2e} (margin alone, relative to itself {rel:.2e})")
    assert dev <= 1e-10, dev


def _mixed():
    """Shape 0's planted agents with a feasible one (3), a NaN state (4) and a NaN model (5)."""
    p0, _, _, _ = reference(0)
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p0.items()}
    p["h"][3] = 50.0
    p["x0"][4, 1] = np.nan
    p["A"][5, 1, 0, 0] = np.nan
    return p


def test_no_certificate_and_status_selects_the_agents(gpu_ctx):
    import torch

    from cmpc import infeas

    p = _mixed()
    B = p["A"].shape[0]
    ref = infeas.certify_rows(p)
    got = infeas.certify_rows_gpu(p, ctx=gpu_ctx)
    assert list(ref["status"]) == [-3, -3, -3, 0, 0, 0]
    for k in ("status", "iters", "nrows"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    assert got["margin"][3] == 0.0 and np.isnan(got["margin"][4:]).all() and np.isnan(got["ray"][3:]).all()
    assert got["iters"][4] == infeas.CERT_ROWS_CHECK_EVERY and got["iters"][5] == 0
    # status 1, 2 and -3 are skipped with nothing written; max_iter / check_every reach the kernel
    st = np.array([1, 2, -3, -2, -10, 0], np.int32)
    q = reference(0)[0]
    ref = infeas.certify_rows(q, st, max_iter=12, check_every=4)
    got = infeas.certify_rows_gpu(q, st, max_iter=12, check_every=4, ctx=gpu_ctx)
    assert list(got["status"]) == list(ref["status"]) and list(got["status"][:3]) == [1, 2, -3]
    assert np.array_equal(got["iters"], ref["iters"]) and (got["iters"][:3] == 0).all()
    assert (got["iters"][3:] % 4 == 0).all() and (got["iters"][3:] <= 12).all()
    assert np.isnan(got["ray"][:3]).all() and np.isnan(got["margin"][:3]).all()
    # the device entry point on resident tensors: the same outputs, bit for bit
    dev = torch.device("cuda", gpu_ctx.device)
    d = {k: torch.from_numpy(np.ascontiguousarray(q[k], dtype=np.float64)).to(dev) for k in ("A", "B", "x0", "C", "h")}
    host = infeas.certify_rows_gpu(q, st, ctx=gpu_ctx)
    std = torch.from_numpy(st.copy()).to(dev)
    ray = torch.full((B, host["ray"].shape[1]), float("nan"), dtype=torch.float64, device=dev)
    margin = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    iters = torch.zeros((B,), dtype=torch.int32, device=dev)
    nrows = torch.zeros((B,), dtype=torch.int32, device=dev)
    infeas.certify_rows_dev(q, d, std, ray, margin, iters, nrows, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert np.array_equal(std.cpu().numpy(), host["status"]) and np.array_equal(iters.cpu().numpy(), host["iters"])
    assert np.array_equal(nrows.cpu().numpy(), host["nrows"])
    assert np.array_equal(ray.cpu().numpy(), host["ray"], equal_nan=True)
    assert np.array_equal(margin.cpu().numpy(), host["margin"], equal_nan=True)
    assert (host["status"][3:] == -3).all() and np.isfinite(host["ray"][3:]).all()


def _di_mixed():
    """The double-integrator batch of tests/test_infeas_gpu.py (agent 0 single-row infeasible, agent 1 a NaN
    state) with agent 2's minimum-speed rows of stages 5 and 6 contradicting each other."""
    H = _di_with_an_infeasible_and_a_nan_agent()
    H["C"] = H["C"].copy()
    plant_consecutive(H, 2, 5, 0)
    return H


@pytest.mark.parametrize("path", [dict(), dict(generic=True), dict(riccati=True), dict(rescue=True, polish=True)],
                         ids=["default", "generic", "riccati", "rescue_polish"])
def test_solve_with_the_flag(gpu_ctx, path):
    """Status -3 for the combined-infeasible agent behind every solver path with certify="rows", not with
    certify=True; everything else bit for bit what the same call returns with certify=True and without."""
    import cmpc
    from cmpc import infeas

    H = _di_mixed()
    assert list(infeas.certify(H)["row"][:3]) == [0, -1, -1]
    z0, k0, i0, s0 = cmpc.solve_mpc(H, gpu_ctx, max_iter=40, **path)
    z1, k1, i1, s1 = cmpc.solve_mpc(H, gpu_ctx, max_iter=40, certify=True, **path)
    z, kkt, it, st = cmpc.solve_mpc(H, gpu_ctx, max_iter=40, certify="rows", **path)
    print(f"statuses: off {s0}, single {s1}, rows {st}")
    assert s0[2] not in (1, 2, -3) and s1[2] == s0[2]
    assert st[0] == -3 and s1[0] == -3 and st[2] == -3, st
    assert st[1] not in (1, 2, -3) and (st[3:] == 1).all(), st
    for zz, kk, ii in ((z0, k0, i0), (z1, k1, i1)):
        assert np.array_equal(z, zz, equal_nan=True) and np.array_equal(kkt, kk, equal_nan=True)
        assert np.array_equal(it, ii)
    assert np.array_equal(np.delete(st, [0, 2]), np.delete(s0, [0, 2])) and np.array_equal(np.delete(st, 2), np.delete(s1, 2))


def test_flag_bits_and_argument_checks(gpu_ctx):
    import torch

    import cmpc
    from cmpc import _lib as L
    from cmpc.solver import _dims, _weights

    H = _di_mixed()
    _, _, _, st = cmpc.solve_mpc(H, gpu_ctx, max_iter=40, flags=4096 | 8192)
    assert st[0] == -3 and st[2] == -3
    with pytest.raises(cmpc.CmpcError) as ei:            # ROWS without CERTIFY
        cmpc.solve_mpc(H, gpu_ctx, max_iter=40, flags=8192)
    assert ei.value.code == L.CMPC_ERR_ARG
    with pytest.raises(ValueError):
        cmpc.solve_mpc(H, gpu_ctx, certify="row")
    # the device solve: the same statuses
    dev = torch.device("cuda", gpu_ctx.device)
    d = {k: torch.from_numpy(np.ascontiguousarray(H[k], dtype=np.float64)).to(dev) for k in cmpc.solver.PER_AGENT}
    out = dict(z=torch.zeros((8, cmpc.nz_of(H)), dtype=torch.float64, device=dev),
               status=torch.zeros(8, dtype=torch.int32, device=dev))
    cmpc.solve_mpc_dev(H, d, out, gpu_ctx, max_iter=40, certify="rows")
    torch.cuda.synchronize()
    assert np.array_equal(out["status"].cpu().numpy(), st)
    # the argument checks of the certificate entry points
    lib = gpu_ctx.lib
    assert lib.cmpc_mpc_certify_rows(gpu_ctx.h, None, None, None, None, None, 0, 0) == L.CMPC_ERR_ARG
    assert lib.cmpc_mpc_certify_rows_dev(gpu_ctx.h, None, None, None, None, None, 0, 0, None) == L.CMPC_ERR_ARG
    w, keep = _weights(H)
    arrs = [L.f64(H[k]) for k in ("A", "B", "x0", "u_prev", "qlin", "C", "h")]
    data = L.cmpc_mpc_data(*[L.dptr(a) for a in arrs])
    none = L.cmpc_mpc_cert_rows(None, None, None, None)
    assert lib.cmpc_mpc_certify_rows(gpu_ctx.h, ct.byref(_dims(H, 8)), ct.byref(w), ct.byref(data), None, None, 0,
                                     0) == L.CMPC_ERR_ARG
    nodata = L.cmpc_mpc_data(None, None, None, None, None, None, None)
    assert lib.cmpc_mpc_certify_rows(gpu_ctx.h, ct.byref(_dims(H, 8)), ct.byref(w), ct.byref(nodata), None,
                                     ct.byref(none), 0, 0) == L.CMPC_ERR_ARG
    assert lib.cmpc_mpc_certify_rows(gpu_ctx.h, ct.byref(_dims(H, 0)), ct.byref(w), ct.byref(data), None,
                                     ct.byref(none), 0, 0) == L.CMPC_OK
    assert lib.cmpc_mpc_certify_rows_dev(gpu_ctx.h, ct.byref(_dims(H, 0)), ct.byref(w), ct.byref(nodata), None,
                                         ct.byref(none), 0, 0, None) == L.CMPC_OK


def test_drop_in_reports_primal_infeasible_with_the_combined_certificate(gpu_ctx):
    import cmpc
    from cmpc import infeas, structure

    _, c = next(iter(lpv_qps("lpv_n30_a3")))
    p = structure.recognize(*_osqp_args(c))
    p["C"], p["h"] = p["C"].copy(), p["h"].copy()
    plant_consecutive(p, 0, 5, 0)                # the minimum-speed rows of stages 5 and 6
    assert infeas.certify(p)["row"][0] == -1
    P, q, G, h, A, b = structure.reference_form(p, 0)
    res0, feas0 = cmpc.osqp_solve_qp(P, q, G, h, A, b, ctx=gpu_ctx)
    z0, _, _, s0 = cmpc.solve_mpc(p, gpu_ctx, rescue=True, polish=True, certify=True)
    # without the keyword: what the adapter returns today
    assert res0.info.status_val == int(s0[0]) != -3 and res0.prim_inf_cert is None
    assert np.array_equal(res0.x, z0[0], equal_nan=True)
    res, feasible = cmpc.osqp_solve_qp(P, q, G, h, A, b, ctx=gpu_ctx, certify_rows=True)
    assert res.info.solver == "structured"
    assert res.info.status_val == -3 and res.info.status == "primal infeasible" and feasible == 0
    assert np.array_equal(res.x, res0.x, equal_nan=True)
    y = res.prim_inf_cert
    assert y is not None and y.shape == (G.shape[0] + A.shape[0],)
    r, gap = infeas.verify(G, h, A, b, y)
    print(f"drop-in: residual {r:.2e} gap {gap:.4f} |y|inf {np.abs(y).max():.2e}")
    assert r <= 1e-12 * np.abs(y).max() and gap < 0 and (y[:G.shape[0]] >= 0).all()
