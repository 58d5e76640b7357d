"""`scenarios.order_by_iters`, the numpy statement of the device launch order (cmpc_order_by_iters_dev):
descending min(max(iters, 0), 65535), equal keys in index order."""
import numpy as np
import pytest

from cmpc import scenarios as S


@pytest.mark.parametrize("n,hi", [(1, 60), (65, 60), (1000, 60), (1000, 700), (4096, 65535)])
def test_in_range_keys_equal_torch_stable_descending_argsort(n, hi):
    import torch

    it = np.random.default_rng(n + hi).integers(0, hi + 1, n).astype(np.int32)
    want = torch.argsort(torch.as_tensor(it), descending=True, stable=True).to(torch.int32).numpy()
    got = S.order_by_iters(it)
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_equal_keys_keep_index_order():
    assert np.array_equal(S.order_by_iters(np.full(100, 7, np.int32)), np.arange(100))
    assert np.array_equal(S.order_by_iters(np.zeros(0, np.int32)), np.zeros(0, np.int32))
    it = np.array([3, 9, 3, 9, 1, 3], np.int32)
    assert np.array_equal(S.order_by_iters(it), [1, 3, 0, 2, 5, 4])
    assert np.array_equal(S.order_by_iters(np.arange(50, dtype=np.int32)), np.arange(50)[::-1])


def test_keys_are_clamped_to_16_bits():
    # negative counts tie with 0, counts above 65535 tie with 65535: ties in index order
    it = np.array([-5, 0, 70000, 65535, -(2 ** 31), 2 ** 31 - 1, 65534, 1], np.int32)
    assert np.array_equal(S.order_by_iters(it), [2, 3, 5, 6, 7, 0, 1, 4])
    assert sorted(S.order_by_iters(it)) == list(range(8))
