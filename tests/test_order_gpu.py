"""cmpc_order_by_iters_dev (cmpc.rounds.order_by_iters_dev) against its numpy statement
`scenarios.order_by_iters`: the result is fully determined, so equal integers.  The kernel is one workgroup
of up to 1024 threads walking tiles of its size: 1 .. 1000 launch fewer wavefronts, 1025 and 8193 take more
than one tile with a ragged last one."""
import ctypes as ct

import numpy as np
import pytest

from cmpc import scenarios as S

pytestmark = pytest.mark.gpu

BATCHES = [1, 63, 64, 65, 1000, 1025, 8193]


def keys(pattern, n):
    rng = np.random.default_rng(1000 * n + len(pattern))
    if pattern == "equal":
        return np.full(n, 17, np.int32)
    if pattern == "increasing":
        return np.arange(n, dtype=np.int32)
    if pattern == "low":                      # one digit
        return rng.integers(0, 61, n).astype(np.int32)
    if pattern == "two_digits":               # the second digit decides too
        return rng.integers(0, 701, n).astype(np.int32)
    assert pattern == "clamped"               # negative and > 65535 mixed in: clamp ties, in index order
    it = rng.integers(0, 701, n).astype(np.int64)
    pick = rng.integers(0, 6, n)
    it = np.where(pick == 0, -rng.integers(1, 2 ** 31, n), it)
    it = np.where(pick == 1, 65536 + rng.integers(0, 2 ** 30, n), it)
    it = np.where(pick == 2, 65535 - rng.integers(0, 3, n), it)
    return it.astype(np.int32)


@pytest.mark.parametrize("pattern", ["equal", "increasing", "low", "two_digits", "clamped"])
@pytest.mark.parametrize("n", BATCHES)
def test_order_equals_numpy_statement(gpu_ctx, n, pattern):
    import torch

    from cmpc.rounds import order_by_iters_dev

    it = keys(pattern, n)
    out = torch.full((n,), -1, dtype=torch.int32, device="cuda")   # an entry the kernel leaves out stays -1
    got = order_by_iters_dev(torch.as_tensor(it, device="cuda"), out=out, ctx=gpu_ctx).cpu().numpy()
    assert got.dtype == np.int32
    assert np.array_equal(np.sort(got), np.arange(n)), "not a permutation"
    assert np.array_equal(got, S.order_by_iters(it))
    if pattern == "equal":
        assert np.array_equal(got, np.arange(n))
    if pattern == "increasing":
        assert np.array_equal(got, np.arange(n)[::-1])


def test_out_argument_and_smaller_batch_after_larger(gpu_ctx):
    """`out` is written in place; a smaller batch after a larger one reuses the context's scratch."""
    import torch

    from cmpc.rounds import order_by_iters_dev

    for n in (3000, 130):
        it = keys("two_digits", n)
        out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        assert order_by_iters_dev(torch.as_tensor(it, device="cuda"), out=out, ctx=gpu_ctx) is out
        assert np.array_equal(out.cpu().numpy(), S.order_by_iters(it))


def test_matches_torch_argsort_on_iteration_counts(gpu_ctx):
    """What DIRounds builds with torch: the same permutation for keys in range."""
    import torch

    from cmpc.rounds import order_by_iters_dev

    it = torch.as_tensor(keys("low", 1025), device="cuda")
    want = torch.argsort(it, descending=True, stable=True).to(torch.int32)
    assert torch.equal(order_by_iters_dev(it, ctx=gpu_ctx), want)


def test_empty_batch_and_argument_errors(gpu_ctx):
    import torch

    from cmpc import _lib as L
    from cmpc.rounds import order_by_iters_dev

    fn, h = gpu_ctx.lib.cmpc_order_by_iters_dev, gpu_ctx.h
    it = torch.zeros(8, dtype=torch.int32, device="cuda")
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = lambda t, o=0: ct.cast(ct.c_void_p(t.data_ptr() + 4 * o), L._IP)  # noqa: E731
    assert fn(h, 0, None, None, None) == L.CMPC_OK                        # nothing to do, nothing launched
    assert order_by_iters_dev(it[:0], ctx=gpu_ctx).shape == (0,)
    assert fn(h, -1, p(it), p(out), None) == L.CMPC_ERR_ARG
    assert fn(h, 8, None, p(out), None) == L.CMPC_ERR_ARG
    assert fn(h, 8, p(it), None, None) == L.CMPC_ERR_ARG
    assert fn(h, 8, p(it), p(it), None) == L.CMPC_ERR_ARG                 # in place
    assert fn(h, 4, p(it), p(it, 3), None) == L.CMPC_ERR_ARG              # overlapping
    assert fn(None, 8, p(it), p(out), None) == L.CMPC_ERR_ARG
    assert fn(h, 4, p(it), p(it, 4), None) == L.CMPC_OK                   # adjacent halves of one buffer
    torch.cuda.synchronize()
    with pytest.raises(L.CmpcError):
        order_by_iters_dev(it, out=it, ctx=gpu_ctx)
    for bad in (it.to(torch.int64), it.cpu(), it.reshape(2, 4), torch.zeros(16, dtype=torch.int32, device="cuda")[::2]):
        with pytest.raises(ValueError):
            order_by_iters_dev(bad, ctx=gpu_ctx)
    for bad in (out[:4], out.to(torch.int64), out.cpu()):
        with pytest.raises(ValueError):
            order_by_iters_dev(it, out=bad, ctx=gpu_ctx)
