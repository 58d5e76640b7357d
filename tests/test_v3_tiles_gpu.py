"""The v3 kernel around the tile counts' edges: horizons whose condensed size n = 2 N leaves fewer than four
padding columns in three tiles (N = 23, 24) run the four-tile instantiation (mpc3_tiles, mpc_ipm3.hip), because
the three-tile one gave wrong Newton directions there.  One fused round of eight agents with a dense time-invariant
model (the perturbed population of test_v3_lti_gpu) at N = 22 .. 25, against the C oracle: every agent solved
on both sides and z within 1e-6, the bar smoke() holds the synthetic batch to (the wrong directions ended at
status -10 / -2 and 1e-3 from the oracle; a sound solve agrees to 1e-13)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [22, 23, 24, 25])
def test_round_matches_oracle_around_three_tiles(gpu_ctx, N):
    import torch
    from cmpc import scenarios as S
    from cmpc.rounds import DIRounds
    from oracle import cmpc_oracle as CO
    from oracle import synth
    from test_v3_lti_gpu import perturbed

    sc = perturbed(S.make_di(8, N, 2, 2))
    P = synth.structured(sc.shared, sc.params, sc.A, sc.B, sc.x0, sc.u_prev, sc.lane, sc.nbr, sc.traj, np.arange(8))
    zc, _, _, stc = CO.solve_batch(P)
    assert (stc == 1).all()
    for lti in (False, True):
        R = DIRounds(sc, ctx=gpu_ctx, lti=lti)
        R.step()
        torch.cuda.synchronize()
        assert (R.status.cpu().numpy() == 1).all(), (lti, R.status)
        assert np.abs(R.z.cpu().numpy() - zc).max() < 1e-6, lti
