"""Host side of the rounds' device log (no GPU): the numpy statement of a round's log rows
(cmpc.scenarios.log_row), the reference's csv/<id>/*.dat files from a log dict (cmpc.logio.save_run), and the
C boundary's declarations (cmpc_round_log_dev, cmpc_*_rounds_log_*)."""
import os
import re

import numpy as np
import pytest

from cmpc import _lib as L
from cmpc import logio
from cmpc import scenarios as S

FILES = ("states.dat", "u.dat", "plan_dist.dat", "time.dat")


def test_log_row_on_a_hand_built_z():
    """z[b, i] = 1000 b + i, so every entry names its own place: nx, nu, ns, N = 3, 2, 1, 2 has stages of 4
    doubles, xPred[0] at 0..2, xPred[-1] at 8..10, uPred[0] at 12..13, nz = 12 + 8."""
    nx, nu, ns, N = 3, 2, 1, 2
    nz = (nx + ns) * (N + 1) + 2 * nu * N
    assert nz == 20
    z = 1000.0 * np.arange(3)[:, None] + np.arange(nz)[None, :]
    z[:, 9] += np.array([0.5, 0.25, 0.125])           # xPred[-1, 1]
    state, u, look = S.log_row(z, nx, nu, ns, N, 1)
    assert np.array_equal(state, z[:, 0:3]) and state.shape == (3, 3)
    assert np.array_equal(u, z[:, 12:14]) and u.shape == (3, 2)
    assert np.array_equal(look, np.array([8.5, 8.25, 8.125])) and look.shape == (3,)
    assert np.array_equal(S.log_row(z, nx, nu, ns, N, 0)[2], np.full(3, 8.0))
    state[0, 0] = -1.0                                 # copies, not views
    assert z[0, 0] == 0.0
    # an agent without a solution: NaN rows, the others untouched
    z[1] = np.nan
    state, u, look = S.log_row(z, nx, nu, ns, N, 2)
    assert np.isnan(state[1]).all() and np.isnan(u[1]).all() and np.isnan(look[1])
    assert np.isfinite(state[[0, 2]]).all() and np.isfinite(look[[0, 2]]).all()
    for bad in (dict(look_col=3), dict(look_col=-1), dict(N=3), dict(ns=2)):
        kw = dict(nx=nx, nu=nu, ns=ns, N=N, look_col=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.log_row(z, **kw)
    # the reference's layout: PlannerLPV's z, nx, nu, ns = 9, 2, 3, s in column 6
    N = 10
    z = np.random.default_rng(5).standard_normal((2, 12 * (N + 1) + 4 * N))
    state, u, look = S.log_row(z, 9, 2, 3, N, 6)
    assert np.array_equal(state, z[:, 0:9]) and np.array_equal(u, z[:, 12 * (N + 1):12 * (N + 1) + 2])
    assert np.array_equal(look, z[:, 12 * N + 6] - z[:, 6])


def synthetic_log(rounds=4, agents=3, seed=11):
    rng = np.random.default_rng(seed)
    return dict(state=rng.standard_normal((rounds, agents, 9)) * 3.0, u=rng.standard_normal((rounds, agents, 2)),
                look_ahead=rng.uniform(0.1, 2.0, (rounds, agents)), solve_ms=rng.uniform(0.2, 5.0, rounds),
                kkt=rng.uniform(0, 1e-9, (rounds, agents)), iters=np.full((rounds, agents), 9, np.int32),
                status=np.ones((rounds, agents), np.int32))


def test_save_run_writes_what_save_to_csv_writes(tmp_path):
    log = synthetic_log()
    dirs = logio.save_run(str(tmp_path / "run"), log, first_agent_id=5)
    assert [os.path.basename(d) for d in dirs] == ["5", "6", "7"]
    for b in range(3):
        want = logio.save_to_csv(str(tmp_path / "direct"), 5 + b, log["state"][:, b], log["u"][:, b],
                                 log["look_ahead"][:, b], log["solve_ms"] / 1e3)
        assert sorted(os.listdir(dirs[b])) == sorted(FILES)
        for f in FILES:
            got = open(os.path.join(dirs[b], f), "rb").read()
            assert got == open(os.path.join(want, f), "rb").read(), (b, f)
            assert got
    # the default ids start at 0, as the reference's agents
    assert os.path.basename(logio.save_run(str(tmp_path / "zero"), log)[0]) == "0"


def test_save_run_round_trip_and_golden_row_format(tmp_path):
    """np.loadtxt gives the values back to the file format's precision (%.5e: six significant digits), time.dat
    in seconds; a row has the shape of the reference's own files (tests/golden/ref_logs/lpv/csv/0)."""
    from conftest import GOLDEN

    log = synthetic_log()
    d = logio.save_run(str(tmp_path), log)[1]
    for f, want in (("states.dat", log["state"][:, 1]), ("u.dat", log["u"][:, 1]),
                    ("plan_dist.dat", log["look_ahead"][:, 1]), ("time.dat", log["solve_ms"] / 1e3)):
        got = np.loadtxt(os.path.join(d, f))
        assert got.shape == want.shape, f
        # %.5e rounds the sixth significant digit: half a unit of it, relative
        assert np.all(np.abs(got - want) <= 0.5e-5 * np.abs(want) * (1 + 1e-12) + 1e-300), f
        ref = np.loadtxt(os.path.join(GOLDEN, "ref_logs", "lpv", "csv", "0", f))
        assert ref.shape[1:] == got.shape[1:], f
        line = open(os.path.join(d, f)).readline().split()
        assert all(re.fullmatch(r"-?\d\.\d{5}e[+-]\d{2}", t) for t in line), line


def declared(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(cmpc_\w+)\s*\(", src, flags=re.M))


LOG_FUNCTIONS = ["cmpc_round_log_dev"] + [f"cmpc_{fam}_rounds_log_{op}" for fam in ("lpv", "di")
                                          for op in ("enable", "range", "read")]


def test_header_and_bindings_declare_the_log():
    src = open(L.HEADER).read()
    fns = declared(src)
    for name in LOG_FUNCTIONS:
        assert name in fns, name
        assert name in L.SIGNATURES, name
    assert re.search(r"#define\s+CMPC_LOG_SEPARATION\s+1\b", src) and L.CMPC_LOG_SEPARATION == 1
    assert re.search(r"#define\s+CMPC_ABI_VERSION\s+6\b", src)       # additions only
    for struct in ("cmpc_log_dims", "cmpc_log_row", "cmpc_rounds_log"):
        assert re.search(r"}\s*" + struct + r"\s*;", src), struct
    assert [f for f, _ in L.cmpc_log_dims._fields_] == ["batch", "nx", "nu", "ns", "N", "look_col"]
    assert [f for f, _ in L.cmpc_log_row._fields_] == ["state", "u", "look_ahead", "kkt", "iters", "status"]
    assert [f for f, _ in L.cmpc_rounds_log._fields_] == ["state", "u", "look_ahead", "kkt", "iters", "status", "sep2",
                                                          "nearest", "solve_ms"]
    lib = L.load()
    for name in LOG_FUNCTIONS:
        assert hasattr(lib, name), name


def test_null_handles_are_argument_errors():
    """No handle, no context, no device: every log entry point refuses a NULL handle."""
    lib = L.load()
    assert lib.cmpc_round_log_dev(None, None, None, None, None, None, None, None) == L.CMPC_ERR_ARG
    for fam in ("lpv", "di"):
        assert getattr(lib, f"cmpc_{fam}_rounds_log_enable")(None, 4, 0) == L.CMPC_ERR_ARG
        assert getattr(lib, f"cmpc_{fam}_rounds_log_range")(None, None, None) == L.CMPC_ERR_ARG
        assert getattr(lib, f"cmpc_{fam}_rounds_log_read")(None, 0, 0, None) == L.CMPC_ERR_ARG
