"""cmpc_di_round_dev (the fused launch also advances the round: x0 <- x_1, u_prev <- u_0, traj_local <- the
predicted positions, from the solver's epilogue) against cmpc_di_solve_dev + cmpc_di_advance_dev: every
output and every piece of round state bit for bit."""
import pytest

pytestmark = pytest.mark.gpu

STATE = ("z", "kkt", "iters", "status", "x0", "u_prev", "traj_local", "traj_all")


def _compare(gpu_ctx, n, N, nb, rounds):
    import torch
    from cmpc import scenarios as S
    from cmpc.rounds import DIRounds

    sc = S.make_di(n, N, nb, 2)
    A = DIRounds(sc, ctx=gpu_ctx)   # step(): cmpc_di_round_dev, then the exchange
    B = DIRounds(sc, ctx=gpu_ctx)   # two launches: build_solve(), advance(); then the exchange
    for rnd in range(rounds):
        A.step()
        B.build_solve()
        B.advance()
        B.exchange()
        torch.cuda.synchronize()
        for a in STATE:
            assert torch.equal(getattr(A, a), getattr(B, a)), (rnd, a)
    assert (B.status == 1).double().mean().item() >= 0.99


@pytest.mark.parametrize("n,N,nb", [(6, 9, 2), (6, 30, 2)])
def test_round_entry_bit_equal_to_solve_then_advance(gpu_ctx, n, N, nb):
    _compare(gpu_ctx, n, N, nb, 3)


def test_round_entry_more_workgroups_than_resident(gpu_ctx):
    """4096 workgroups on a device that holds 1024 at a time: the late ones build their rows from traj_all
    after the early ones have finished, so a write to traj_all from inside the launch would change them."""
    _compare(gpu_ctx, 4096, 9, 2, 1)
