"""The fused row-broadcast fma of the v3 kernel (wave_ops.h: v_fmac_f64 with a DPP row_newbcast
source, written as inline asm) against the two-instruction expression it replaces.

One wavefront evaluates both on the same inputs for every broadcast lane J in 0..15, both signs
and both forms (self-contained, settled source), with the broadcast source written by the
instruction directly in front: the read-after-write case that the compiler no longer pads.  The
fused form is the same single-rounded fma on the same operands, so the results must be equal bit
for bit; where the expression gives a NaN the fused form must give a NaN.
"""
import numpy as np
import pytest

TINY = np.finfo(np.float64).tiny          # smallest normal
DENORM = 5e-324                           # smallest denormal
SPECIALS = np.array([0.0, -0.0, DENORM, -DENORM, TINY / 4, -TINY / 2, np.inf, -np.inf, np.nan,
                     np.finfo(np.float64).max, -TINY, 1.0])


def _inputs(seed):
    """Seeded doubles over many binades; the specials sit at other lanes in each of A, X, C and move
    with the seed, so every J broadcasts a special at some seed and meets specials in A and C."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(3):
        v = rng.standard_normal(64) * 2.0 ** rng.integers(-40, 40, 64)
        lanes = (np.arange(len(SPECIALS)) * 5 + 7 * seed + 3 * k) % 64   # 5 is coprime to 64: distinct lanes
        v[lanes] = SPECIALS
        out.append(v)
    return out


def _assert_bits_equal(fused, ref):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(fused), nan)
    fu, ru = fused.view(np.uint64), ref.view(np.uint64)
    bad = (fu != ru) & ~nan
    assert not bad.any(), [(int(c), int(j), int(l), fused[c, j, l].hex(), ref[c, j, l].hex())
                           for c, j, l in np.argwhere(bad)[:8]]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_fused_broadcast_fma_equals_the_expression(gpu_ctx, seed):
    import cmpc

    A, X, C = _inputs(seed)
    fused, ref = cmpc.selftest_fma_bcast(A, X, C, gpu_ctx)
    assert fused.shape == ref.shape == (4, 16, 64)
    _assert_bits_equal(fused, ref)
    # the reference itself against numpy (both sides above broadcast by DPP): lane J of each row of 16
    # reaches the row.  numpy rounds the product and the sum separately, each within eps / 2 of its
    # result, so it is within eps (|product| + |sum|) of the single-rounded fma, plus a denormal's
    # spacing where a result underflows
    eps = np.finfo(np.float64).eps
    rows = np.arange(64) // 16 * 16
    for J in range(16):
        xb = X[rows + J]
        with np.errstate(all="ignore"):
            prod = xb * A
            want = prod + C
            fin = np.isfinite(prod) & np.isfinite(want)
            bound = eps * (np.abs(prod[fin]) + np.abs(want[fin])) + 2 * DENORM
        assert (np.abs(ref[0, J][fin] - want[fin]) <= bound).all(), J


def test_specials_reach_every_lane_class():
    """The inputs' own shape (no GPU work): a NaN, both zeros, denormals and both infinities are in each
    array, at distinct lanes."""
    for seed in range(4):
        for v in _inputs(seed):
            assert np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
            assert (v == 0).sum() == 2 and np.signbit(v[v == 0]).sum() == 1
            assert ((np.abs(v) < TINY) & (v != 0)).sum() == 4
