"""The LPV handles' consensus step, no GPU: the publication's numpy statement (cmpc.scenarios.lpv_publish) against the
linear family's with the LPV constants, its status count, its threshold, the instance makers the GPU tests use, the
step's rule on the CPU (linearise once per step, iterate the coupling), and the library's exports."""
import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S
from lpv_consensus_cases import (ATOL_T, DEFAULTS, GRID, PLANTS, PUBLISH_SHAPES, STATUSES, golden_case, oracle_state,
                                 oracle_step, planted_agent, positions, publish_instance, threshold_instance)

LPV = dict(ix=7, iy=8, min_dist=0.25, wq=5.0)


def same(a, b):
    """Finite entries bit for bit, NaNs in the same places."""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.where(nan, 0.0, a).tobytes() == np.where(nan, 0.0, b).tobytes()


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("shape", PUBLISH_SHAPES)
def test_lpv_publish_is_lin_publish_with_the_lpv_constants(shape, plant):
    N, B, n, off = shape
    z, traj, status, _ = publish_instance(shape, plant)
    z0, traj0 = z.copy(), traj.copy()
    tl, close, delta, not_close, bad = S.lpv_publish(z, N, traj, status, self_offset=off)
    assert np.array_equal(z, z0, equal_nan=True) and np.array_equal(traj, traj0, equal_nan=True)   # arguments left alone
    want = S.lin_publish(LPV, z, 9, 2, 3, N, traj, self_offset=off)
    assert tl.tobytes() == want[0].tobytes() and np.array_equal(close, want[1]) and same(delta, want[2])
    assert not_close == want[3] and close.dtype == np.int32 and tl.shape == (B, N + 1, 2)
    assert bad == sum(int(s) not in (1, 2, -2) for s in status) and isinstance(bad, int)
    # the maker: both verdicts occur (what keeps the GPU comparison from being vacuous), and the plant acts
    if B > 1:
        assert 0 < not_close < B
    t = planted_agent(B)
    new = positions(z, N)
    if plant == "plain":
        assert np.array_equal(close, (np.arange(B) % 3 != 1).astype(np.int32)) and np.isfinite(delta).all()
        assert tl.tobytes() == new.tobytes()
    elif plant in ("z_last_nan", "slack_inf", "u_neg_inf"):
        assert np.isfinite(new[t]).all()                     # the position entries themselves were fine
        assert tl[t].tobytes() == traj[off + t].tobytes() and close[t] == 0 and np.isnan(delta[t])
    elif plant == "prev_nan":
        assert tl[t].tobytes() == new[t].tobytes() and close[t] == 0 and np.isnan(delta[t])
    else:
        assert tl[t].tobytes() == new[t].tobytes() and close[t] == 0 and delta[t] == np.inf
    others = [b for b in range(B) if b != t or plant == "plain"]
    assert np.isfinite(delta[others]).all()


def test_lpv_publish_status_rule_and_shape_errors():
    shape = PUBLISH_SHAPES[1]
    N, B, n, off = shape
    z, traj, _, _ = publish_instance(shape)
    for s in STATUSES:
        bad = S.lpv_publish(z, N, traj, np.full(B, s, np.int32), self_offset=off)[4]
        assert bad == (0 if s in (1, 2, -2) else B), s
    assert S.lpv_publish(z, N, traj, None, self_offset=off)[4] == 0
    assert S.lpv_publish(z, N, traj, np.array([1, -3], np.int32), self_offset=off)[4] == 1
    for kw in (dict(z=z[:, :-1]), dict(z=z[0]), dict(traj=traj[:, :-1]), dict(traj=traj[..., :1]), dict(off=n - B + 1),
               dict(off=-1), dict(status=np.ones(B + 1, np.int32)), dict(status=np.ones((B, 1), np.int32)),
               dict(atol=-1.0), dict(rtol=np.nan)):
        with pytest.raises(ValueError):
            S.lpv_publish(kw.get("z", z), N, kw.get("traj", traj), kw.get("status"), atol=kw.get("atol", 0.01),
                          rtol=kw.get("rtol", 1e-5), self_offset=kw.get("off", off))


@pytest.mark.parametrize("shape", PUBLISH_SHAPES)
def test_lpv_publish_threshold(shape):
    N, B, n, off = shape
    z, traj, status, _ = threshold_instance(shape)
    tl, close, delta, not_close, bad = S.lpv_publish(z, N, traj, status, atol=ATOL_T, rtol=0.0, self_offset=off)
    odd = np.arange(B) % 2 == 1
    assert np.array_equal(close, (~odd).astype(np.int32)) and not_close == int(odd.sum()) and bad == 0
    assert (delta[~odd] == ATOL_T).all() and (delta[odd] == ATOL_T + GRID).all()      # exact: a 2^-10 grid
    assert tl.tobytes() == (traj[off:off + B] + ATOL_T + np.where(
        odd[:, None, None] & (np.arange(N + 1)[None, :, None] == N) & (np.arange(2)[None, None, :] == 1), GRID, 0.0)).tobytes()
    if B > 1:
        assert 0 < not_close < B


def test_fixed_linearisation_settles_a_lone_agent():
    """lpv_n10_a1 has no neighbour: with the model fixed within the step nothing couples the inner rounds, so rounds 2
    and 3 repeat round 1 exactly and the step agrees after the minimum of 3 rounds."""
    case = golden_case("lpv_n10_a1")
    assert case["n"] == 1 and case["nbr"].shape == (1, 0)
    st = oracle_state(case)
    x_last0 = st["x_last"].copy()
    r = oracle_step(case, st, "fixed", co=DEFAULTS)
    assert len(r["trace"]) == 3 and r["agreed"] and r["trace"][1:] == [0, 0]
    assert (r["status"] == 1).all()
    assert r["deltas"][1].tolist() == [0.0] and r["deltas"][2].tolist() == [0.0]
    assert r["deltas"][0][0] > 0.0
    assert r["zs"][2].tobytes() == r["zs"][0].tobytes()
    z = r["zs"][2]
    assert st["x0"].tobytes() == z[:, 12:21].tobytes() and st["x_last"].shape == (1, case["N"], 9)
    assert not np.array_equal(st["x_last"], x_last0[:, 1:])


def test_library_exports_the_lpv_consensus_entries():
    import os
    import re

    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "cmpc.h")).read()
    for name in ("cmpc_lpv_publish_dev", "cmpc_lpv_rounds_step_consensus", "cmpc_lpv_rounds_consensus_read"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    assert lib.cmpc_abi_version() == 6
