"""The consensus step's host statements (cmpc.scenarios.lin_publish, consensus_stop), no GPU: the publication's edge
cases and threshold, the stopping rule against the reference's loop counters (cmpc.ocd.OCDLoopState) exhaustively,
and the library's exports."""
import itertools

import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import scenarios as S
from cmpc.ocd import OCDLoopState
from lin_consensus_cases import ATOL_T, PUBLISH_SHAPES, positions, publish_instance, threshold_instance


def publish(shape, inst, **kw):
    nx, ns, nu, N = shape[:4]
    prm, z, traj, off = inst
    return S.lin_publish(prm, z, nx, nu, ns, N, traj, self_offset=off, **kw)


def test_publish_edge_cases():
    shape = PUBLISH_SHAPES[0]
    nx, ns, nu, N, B, ix, iy, n, off = shape
    inst = publish_instance(shape)
    prm, z, traj, _ = inst
    assert off > 0 and np.isnan(z[0, -1]) and np.isinf(z[1, nx]) and np.isnan(traj[off + 2, 1, 0])
    z0, traj0 = z.copy(), traj.copy()
    tl, close, delta, not_close = publish(shape, inst)
    assert np.array_equal(z, z0, equal_nan=True) and np.array_equal(traj, traj0, equal_nan=True)   # arguments left alone
    assert tl.shape == (B, N + 1, 2) and close.dtype == np.int32 and close.shape == delta.shape == (B,)
    new = positions(shape, z)
    # a NaN in the last du entry, an inf in a slack entry: the row of the exchange buffer again, bit for bit
    for b in (0, 1):
        assert tl[b].tobytes() == traj[off + b].tobytes() and close[b] == 0 and np.isnan(delta[b])
        assert np.isfinite(new[b]).all()                     # the position entries themselves were fine
    # a NaN in prev: published, never close, delta NaN (numpy's max)
    assert tl[2].tobytes() == new[2].tobytes() and close[2] == 0 and np.isnan(delta[2])
    # -0.0 kept; close (moved by at most 0.005 < atol)... agent 3 is odd: moved by up to 0.05
    assert np.signbit(tl[3, 1, 0]) and np.signbit(tl[3, 2, 1]) and tl[3, 1, 0] == 0.0
    assert tl[3].tobytes() == new[3].tobytes() and tl[4].tobytes() == new[4].tobytes()
    assert close[3] == 0 and 0.01 < delta[3] <= 0.05
    assert close[4] == 1 and 0.0 < delta[4] <= 0.005
    assert delta[4] == np.abs(traj[off + 4] - new[4]).max()
    assert not_close == 4 and isinstance(not_close, int)


@pytest.mark.parametrize("shape", PUBLISH_SHAPES)
def test_publish_threshold(shape):
    B = shape[4]
    inst = threshold_instance(shape)
    tl, close, delta, not_close = publish(shape, inst, atol=ATOL_T, rtol=0.0)
    odd = np.arange(B) % 2 == 1
    assert np.array_equal(close, (~odd).astype(np.int32)) and not_close == int(odd.sum())
    assert (delta[~odd] == 0.25).all() and (delta[odd] == np.nextafter(1.25, 2.0) - 1.0).all()
    assert (delta[odd] > 0.25).all()
    assert (tl[~odd] == 1.25).all()
    # +inf tolerances are taken; a finite z is then close whatever it holds
    assert publish(shape, inst, atol=np.inf, rtol=0.0)[1].all()


def test_publish_shape_errors():
    shape = PUBLISH_SHAPES[0]
    nx, ns, nu, N, B, ix, iy, n, off = shape
    prm, z, traj, _ = publish_instance(shape)
    bad = [dict(z=z[:, :-1]), dict(z=z[0]), dict(traj=traj[:, :-1]), dict(traj=traj[..., :1]), dict(traj=traj[0]),
           dict(off=n - B + 1), dict(off=-1), dict(prm=dict(prm, ix=nx)), dict(prm=dict(prm, iy=-1)),
           dict(prm=dict(prm, ix=1, iy=1)), dict(atol=-1.0), dict(rtol=-1e-9), dict(atol=np.nan), dict(rtol=np.nan)]
    for kw in bad:
        with pytest.raises(ValueError):
            S.lin_publish(kw.get("prm", prm), kw.get("z", z), nx, nu, ns, N, kw.get("traj", traj),
                          atol=kw.get("atol", 0.01), rtol=kw.get("rtol", 1e-5), self_offset=kw.get("off", off))
    for kw in (dict(not_close=[]), dict(min_rounds=0), dict(need=0), dict(min_rounds=3, max_rounds=2)):
        args = dict(dict(not_close=[0], min_rounds=1, need=1, max_rounds=4), **kw)
        with pytest.raises(ValueError):
            S.consensus_stop(**args)


def stop_round(seq, min_rounds, need, max_rounds):
    """(the round after which consensus_stop ends the step, agreed) for the close-sequence seq[j-1] of round j"""
    trace = [0 if c else 1 for c in seq]
    for j in range(1, len(seq) + 1):
        stop, agreed = S.consensus_stop(trace[:j], min_rounds, need, max_rounds)
        if stop:
            return j, agreed
    raise AssertionError("no stop within max_rounds")


def ocd_stop_round(seq, min_rounds, need, max_rounds):
    """The same from the reference's counters; agreed = the loop of an unbounded max_it_OCD has finished"""
    st = OCDLoopState(min_rounds - 1, need - 1, max_rounds - 2)
    free = OCDLoopState(min_rounds - 1, need - 1, 10 ** 9)
    j = 0
    while st.running():
        st.after_round(seq[j])
        free.after_round(seq[j])
        j += 1
    return j, free.finished


def test_consensus_stop_is_the_reference_loop():
    seqs = list(itertools.product((False, True), repeat=8))      # every close-sequence of length <= 8 is a prefix
    cases = 0
    for max_rounds in range(1, 9):
        for min_rounds in range(1, max_rounds + 1):
            for need in (1, 2, 3):
                for seq in seqs:
                    got = stop_round(seq, min_rounds, need, max_rounds)
                    assert got == ocd_stop_round(seq, min_rounds, need, max_rounds), (seq, min_rounds, need, max_rounds)
                    assert min(min_rounds, max_rounds) <= got[0] <= max_rounds
                    cases += 1
    assert cases == 36 * 3 * 256
    # the defaults are the reference's (min_it_OCD, it_conv, max_it_OCD) = (2, 1, 10)
    ref = OCDLoopState()
    assert (ref.min_it_OCD + 1, ref.it_conv + 1, ref.max_it_OCD + 2) == (3, 2, 12)
    assert S.consensus_stop([5, 0, 0]) == (True, True) and S.consensus_stop([0, 0]) == (False, False)
    assert S.consensus_stop([5] * 11) == (False, False) and S.consensus_stop([5] * 12) == (True, False)


def test_library_exports_the_consensus_entries():
    lib = L.load()
    for name in ("cmpc_lin_publish_dev", "cmpc_lin_rounds_step_consensus", "cmpc_lin_rounds_consensus_read"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert lib.cmpc_abi_version() == 6
