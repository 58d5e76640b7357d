"""cmpc.rounds.is_lti, the host test behind CMPC_FLAG_LTI: every stage of an agent's A and B bit-equal to its
stage 0, compared as 64-bit patterns, and every entry finite (what DIRounds runs by default, and what
cmpc_di_rounds_create restates in C on its host arrays)."""
import numpy as np
import pytest

from cmpc import scenarios as S
from cmpc.rounds import is_lti


def _ab(n=3, N=5):
    sc = S.make_di(n, N, 2, 2)
    return sc.A.copy(), sc.B.copy()


def test_equal_stages():
    A, B = _ab()
    assert is_lti(A, B)
    rng = np.random.default_rng(1)   # per-agent models differ; the stages of each do not
    A = np.ascontiguousarray(np.broadcast_to(rng.standard_normal((3, 1, 4, 4)), A.shape))
    assert is_lti(A, B)


@pytest.mark.parametrize("which", ["A", "B"])
def test_one_ulp_in_one_entry(which):
    A, B = _ab()
    M = A if which == "A" else B
    M[1, 3, 2, 1] = np.nextafter(M[1, 3, 2, 1], np.inf)
    assert not is_lti(A, B)


def test_negative_zero_is_not_positive_zero():
    A, B = _ab()
    assert A[0, 2, 2, 0] == 0.0 and not np.signbit(A[0, 2, 2, 0])
    A[0, 2, 2, 0] = -0.0
    assert (A == A[:, :1]).all()      # equal as values
    assert not is_lti(A, B)
    A, B = _ab()
    A[:, :, 2, 0] = -0.0              # the same sign at every stage: time-invariant
    assert is_lti(A, B)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("which", ["A", "B"])
def test_non_finite_anywhere(which, bad):
    A, B = _ab()
    M = A if which == "A" else B
    M[2, :, 1, 1] = bad               # at every stage alike: still not LTI
    assert not is_lti(A, B)
    A, B = _ab()
    (A if which == "A" else B)[0, 0, 0, 0] = bad
    assert not is_lti(A, B)


def test_single_stage():
    A, B = _ab(N=1)
    assert A.shape[1] == 1 and is_lti(A, B)
