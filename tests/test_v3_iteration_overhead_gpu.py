"""The v3 iteration's reduced forms (mpc_ipm3.hip: invert_diag from the lane's own row, the K build's diagonal
adds from a table built once per solve) against the generic condensed kernel, which shares none of that code.

One fused round through DIRounds on the dense time-invariant population of test_v3_lti_gpu (perturbed make_di,
8 agents) is compared with cmpc.solve_mpc(R.snapshot(), generic=True) under the same iteration cap.  One capped
Newton step shows a wrong K or a wrong block inverse that a converged solve hides.  Horizons: one to four tiles,
with and without padding columns (N = 8, 16 k / 2 have none), so the last-stage factor and the padding identity
are both exercised; both neighbour counts; with and without CMPC_FLAG_LTI.

Tolerance: max |z_v3 - z_generic| over all these shapes, measured on the commit before the reduced forms
(their results are bit for bit that commit's), per cap; the bar is ten times that figure, since the two kernels
round differently:
    max_iter = 1        measured 1.33e-15  (both kernels return the best iterate by merit, taken where an
                                            iteration evaluates its residuals: under this cap the start point
                                            through the forward simulation, before any Newton step)
    max_iter = 2        measured 5.68e-08  (the iterate after one Newton step; largest at N = 30, nb = 0)
    default (converged) measured 7.37e-14, every agent at status 1 on both sides
With the reduced forms every z of every case below is byte for byte the earlier commit's (measured in the same
session), so the figures are theirs as well."""
import functools

import numpy as np
import pytest

from test_v3_lti_gpu import perturbed

pytestmark = pytest.mark.gpu

HORIZONS = [7, 8, 12, 14, 20, 22, 28, 30, 32]
AGENTS = 8
MEASURED = {1: 1.33e-15, 2: 5.68e-8, None: 7.37e-14}   # max |z_v3 - z_generic| per cap (docstring)


def scenario(N, nb):
    from cmpc import scenarios as S

    return perturbed(S.make_di(AGENTS, N, nb, 2))


@functools.lru_cache(maxsize=None)
def reference(N, nb, cap):
    """(problem, z, status) of the generic kernel on round 0's problem; computed once per (N, nb, cap)."""
    import cmpc
    from cmpc.rounds import DIRounds

    ctx = cmpc.default_context(0)
    R = DIRounds(scenario(N, nb), ctx=ctx)
    R.build()
    z, _, _, st = cmpc.solve_mpc(R.snapshot(), ctx, max_iter=cap, generic=True)
    z.setflags(write=False)
    return z, st


def fused_round(N, nb, cap, lti):
    import torch
    from cmpc.rounds import DIRounds

    R = DIRounds(scenario(N, nb), max_iter=cap, lti=lti)
    R.step()
    torch.cuda.synchronize()
    return R.z.cpu().numpy(), R.status.cpu().numpy()


def difference(N, nb, cap, lti):
    zg, sg = reference(N, nb, cap)
    z, st = fused_round(N, nb, cap, lti)
    return float(np.abs(z - zg).max()), st, sg


@pytest.mark.parametrize("cap", [1, 2, None])
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("N", HORIZONS)
def test_fused_round_matches_generic_kernel(gpu_ctx, N, nb, cap):
    for lti in (False, True):
        err, st, sg = difference(N, nb, cap, lti)
        print(f"N {N} nb {nb} cap {cap} lti {lti}: max |z_v3 - z_generic| {err:.3e} status {st} / {sg}")
        assert np.isfinite(err) and err <= 10 * MEASURED[cap], (lti, err)
        if cap is None:
            assert (st == 1).all() and (sg == 1).all(), (lti, st, sg)
