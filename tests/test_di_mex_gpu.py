"""The cmpc_di MEX gateway (colaborativempc-_amd/mex/cmpc_di_mex.c) through its mock-MEX build: a MATLAB
host's loop over the synthetic family's round handle equals cmpc.rounds.DIRoundsHandle bit for bit."""
import ctypes as ct
import os

import numpy as np
import pytest

import mex_harness as MX
from cmpc import _lib as L
from cmpc import scenarios as S

pytestmark = pytest.mark.gpu

DI_MOCK = os.path.join(os.path.dirname(L.LIB_PATH), "libcmpc_di_mex_mock.so")


def call_di(ps, nlhs):
    """cmpc_di(...) on prepared mxArray pointers -> (outputs | None, (err_id, err_msg) | None)."""
    m = MX.lib(DI_MOCK)
    prhs = (ct.c_void_p * len(ps))(*ps)
    plhs = (ct.c_void_p * max(nlhs, 1))()
    if m.mock_call(nlhs, plhs, len(ps), prhs):
        return None, (m.mock_err_id().decode(), m.mock_err_msg().decode())
    return list(plhs), None


def matlab_structs(sc):
    """A make_di scenario in cmpc_di's MATLAB order (agents last: the C layout read backwards)."""
    sh = sc.shared
    P = {k: np.array([float(v)]) for k, v in sc.params.items()}
    P["N"] = np.array([float(sc.N)])
    P.update(Q=sh["Q"], R=sh["R"], dR=sh["dR"], Qs=sh["Qs"], u_ub=sh["u_ub"], u_lb=sh["u_lb"],
             row_slack=sh["row_slack"].astype(float), row_sign=sh["row_sign"].astype(float))
    D = dict(A=sc.A.transpose(3, 2, 1, 0), B=sc.B.transpose(3, 2, 1, 0), x0=sc.x0.T, u_prev=sc.u_prev.T,
             lane=sc.lane[None, :])
    St = dict(nbr=sc.nbr.T.astype(float), traj=sc.traj.transpose(2, 1, 0))
    return P, D, St


def cmd(name, *args):
    return [MX.mx_str(name)] + [a if isinstance(a, int) else MX.mx(a) for a in args]


def test_mex_di_rounds_equal_python_handle(gpu_ctx):
    from cmpc.rounds import DIRoundsHandle

    sc = S.make_di(6, 9, 2, 2)
    n, nz = 6, (4 + 3) * 10 + 2 * 2 * 9
    H = DIRoundsHandle(sc, ctx=gpu_ctx, history=2)
    assert H.step(2) == 2
    want, hist = H.read(), H.history(0, 2)
    want_traj = H.get_traj()
    H.close()

    P, D, St = matlab_structs(sc)
    St["history"] = np.array([2.0])
    out, err = call_di(cmd("rounds_create", MX.mx_struct(P), MX.mx_struct(D), MX.mx_struct(St)), 1)
    assert err is None, err
    hd = MX.values(out[0])
    o, err = call_di(cmd("rounds_step", hd, np.array([2.0])), 1)
    assert err is None and MX.values(o[0])[0] == 2, err
    o, err = call_di(cmd("rounds_read", hd), 7)
    assert err is None, err
    z, st, kkt, it, x0, up, nbr = (MX.values(p) for p in o)
    assert z.reshape(n, nz).tobytes() == want["z"].tobytes()
    assert kkt.tobytes() == want["kkt"].tobytes()
    assert np.array_equal(st, want["status"]) and np.array_equal(it, want["iters"])
    assert x0.reshape(n, 4).tobytes() == want["x0"].tobytes()
    assert up.reshape(n, 2).tobytes() == want["u_prev"].tobytes()
    assert np.array_equal(nbr.reshape(n, 2), want["nbr"])
    o, err = call_di(cmd("rounds_history", hd, np.array([0.0]), np.array([2.0])), 3)
    assert err is None, err
    assert MX.values(o[0]).reshape(2, n).tobytes() == hist["kkt"].tobytes()
    assert np.array_equal(MX.values(o[1]).reshape(2, n), hist["iters"])
    assert np.array_equal(MX.values(o[2]).reshape(2, n), hist["status"])
    o, err = call_di(cmd("rounds_get_traj", hd), 1)
    assert err is None and MX.values(o[0]).reshape(n, 10, 2).tobytes() == want_traj.tobytes()
    _, err = call_di(cmd("rounds_set_traj", hd, sc.traj.transpose(2, 1, 0)), 0)
    assert err is None, err
    # a third round after two: round 0 has left the ring of two
    o, err = call_di(cmd("rounds_step", hd, np.array([1.0])), 1)
    assert err is None and MX.values(o[0])[0] == 1
    _, err = call_di(cmd("rounds_history", hd, np.array([0.0]), np.array([1.0])), 1)
    assert err[0] == "cmpc:solve" and "(-1)" in err[1]
    _, err = call_di(cmd("rounds_destroy", hd), 0)
    assert err is None
    _, err = call_di(cmd("rounds_read", hd), 1)
    assert err[0] == "cmpc:di:args"


def test_mex_di_argument_error_identifiers(gpu_ctx):
    sc = S.make_di(6, 9, 2, 2)
    P, D, St = matlab_structs(sc)

    def create(P=P, D=D, St=St):
        out, err = call_di(cmd("rounds_create", MX.mx_struct(P), MX.mx_struct(D), MX.mx_struct(St)), 1)
        if err is None:
            assert call_di(cmd("rounds_destroy", MX.values(out[0])), 0)[1] is None
        return err

    drop = lambda d, k: {a: b for a, b in d.items() if a != k}  # noqa: E731
    assert create() is None
    for bad in (dict(P=drop(P, "dim")), dict(P=dict(P, dim=np.array([4.0]))), dict(P=dict(P, N=np.array([0.0]))),
                dict(P=dict(P, Q=np.eye(3))), dict(P=dict(P, row_slack=np.zeros(5))), dict(P=drop(P, "u_ub")),
                dict(D=drop(D, "A")), dict(D=dict(D, x0=np.zeros((3, 7)))), dict(D=dict(D, lane=np.zeros(5))),
                dict(D=dict(D, B=D["B"][..., :5])), dict(St=drop(St, "traj")), dict(St=dict(St, nbr=np.zeros(7))),
                dict(St=dict(St, traj=np.zeros((2, 10, 5)))), dict(St=dict(St, nbr=np.zeros((13, 6))))):
        err = create(**bad)
        assert err is not None and err[0] == "cmpc:di:args", (bad.keys(), err)
    # what the gateway cannot see goes to the library: CMPC_ERR_ARG under cmpc:solve
    far = St["nbr"].copy()
    far[0, 0] = 6.0
    for bad in (dict(St=dict(St, nbr=far)), dict(St=dict(St, history=np.array([-1.0]))),
                dict(St=dict(St, n_total=np.array([12.0]), traj=np.zeros((2, 10, 12))))):   # sharded, no exchange
        err = create(**bad)
        assert err is not None and err[0] == "cmpc:solve" and "(-1)" in err[1], err
    for ps in (cmd("rounds_step", np.array([99.0]), np.array([1.0])), cmd("rounds_history", np.array([1.0])),
               cmd("rounds_create", MX.mx_struct(P)), cmd("no_such_command"), [MX.mx(np.array([1.0]))],
               cmd("rounds_destroy", np.array([0.0])), cmd("comm_init", np.array([1.0]))):
        _, err = call_di(ps, 1)
        assert err is not None and err[0] == "cmpc:di:args", err
