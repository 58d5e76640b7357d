"""The quadprog contract of the dense QP batch (cmpc_solve_qp_batch, include/cmpc.h): the four
multiplier arrays, fval and residual, every exit flag, absent arguments and outputs, infinite
and fixed bounds, the symmetric part of H, the column-major mode and batch isolation.

Reference: the KKT-certified oracle IPM (oracle/qp_ipm.py) on the stacked form
rows = [A; Aeq; I], lo = [-inf; beq; lb], hi = [b; beq; ub].  Its OSQP-convention y maps to
quadprog's multipliers as ineqlin = y[:mi], eqlin = y[mi:mi+me], upper = max(y_box, 0),
lower = max(-y_box, 0) (eqlin has y's sign: test_qp_gpu.test_unconstrained_and_box_known_answers
pins that sign analytically).  The second, independent check is the oracle's residual evaluator
applied to the GPU's own (x, lambda): it needs no uniqueness of the multipliers."""
import ctypes as ct
import functools

import numpy as np
import pytest

from conftest import KKT_TOL
from test_qp_gpu import X_TOL, _rand_qp

pytestmark = pytest.mark.gpu

# Tolerance passed where x is held to X_TOL.  An interior-point iterate with complementarity mu sits
# about mu / margin away from a constraint whose multiplier (or gap) is `margin`, and the kernel stops
# at merit = max(res_d, res_p, mu) < tol.  The reference margins of this family go down to 8e-3, and
# the constraint geometry amplifies further (|x - x*| is roughly 1e3 x the merit at n = 64): the default
# 1e-9 is too close to X_TOL = 1e-6, so half of it is passed.  (At n = 260 the kernel's rounding floor
# is near 3e-10, so much less cannot be asked of `residual < tol`.)
TOL = 5e-10
MARGIN = 1e-3       # strict complementarity the direct multiplier comparison needs of the reference
# Direct comparison |lambda_gpu - lambda_ref|_inf / max(1, |lambda_ref|_inf), per array.  Largest
# deviation measured on an MI355X over SHAPES, the badly scaled family, the semidefinite and the
# fixed-variable problems: ineqlin 1.49e-6 (n = 260), eqlin 3.47e-7 (n = 260), lower 8.8e-10 and
# upper 6.0e-10 (both on the badly scaled family, in the conditioned variable).  Each bar is ten times
# its array's figure rounded up to a power of ten; none may be looser than 1e-4.
LAM_TOL = dict(ineqlin=1e-4, eqlin=1e-5, lower=1e-8, upper=1e-8)
assert max(LAM_TOL.values()) <= 1e-4


def _assert_lam_dev(dev):
    for key, bar in LAM_TOL.items():
        assert dev[key] < bar, (key, dev)


SHAPES = [(0, 1, 1, 0), (1, 2, 3, 1), (2, 8, 6, 2), (3, 20, 15, 5), (4, 40, 30, 0), (5, 30, 0, 10), (6, 64, 80, 8),
          (7, 260, 270, 3)]


# ---------------------------------------------------------------- problems and the reference
def _stacked(p):
    H, f, A, b, Aeq, beq, lb, ub = p
    n = H.shape[0]
    rows = np.vstack([A.reshape(-1, n), Aeq.reshape(-1, n), np.eye(n)])
    lo = np.hstack([np.full(len(b), -np.inf), beq, lb])
    hi = np.hstack([b, beq, ub])
    return rows, lo, hi


def _split(y, n, mi, me):
    yb = y[mi + me:]
    return dict(ineqlin=y[:mi], eqlin=y[mi:mi + me], lower=np.maximum(-yb, 0.0), upper=np.maximum(yb, 0.0))


def _reference(p, **kw):
    """Oracle solve of one problem: (x, lambda dict, certificate, strict-complementarity margin).  The
    margin is the minimum over the one-sided constraints (rows of A, finite lb_i, finite ub_i; a
    fixed variable lb_i = ub_i is an equality) of max(gap, multiplier)."""
    from oracle import qp_ipm

    H, f, A, b, Aeq, beq, lb, ub = p
    n, mi, me = H.shape[0], len(b), len(beq)
    rows, lo, hi = _stacked(p)
    ref = qp_ipm.solve_qp(0.5 * (H + H.T), f, rows, lo, hi, **kw)
    lam = _split(ref.y, n, mi, me)
    A2 = A.reshape(-1, n)
    nz = np.abs(A2).sum(1) > 0
    free = lb != ub
    with np.errstate(invalid="ignore"):
        pairs = [((b - A2 @ ref.x)[nz], lam["ineqlin"][nz]),
                 ((ub - ref.x)[np.isfinite(ub) & free], lam["upper"][np.isfinite(ub) & free]),
                 ((ref.x - lb)[np.isfinite(lb) & free], lam["lower"][np.isfinite(lb) & free])]
    margin = min([float(np.maximum(g, np.abs(y)).min()) for g, y in pairs if len(g)], default=np.inf)
    return ref.x, lam, ref.kkt, margin


def _draw(rng, n, mi, me):
    H, f, *rest = _rand_qp(rng, n, mi, me)
    return (H, 3.0 * f, *rest)   # f x 3: a third to a half of the inequality rows end up active


@functools.lru_cache(maxsize=None)
def _family(seed, n, mi, me, count):
    """`count` problems drawn consecutively from default_rng(100 + seed), each with its reference
    (computed once and shared; callers must not write into it)."""
    rng = np.random.default_rng(100 + seed)
    probs = [_draw(rng, n, mi, me) for _ in range(count)]
    kw = dict(max_iter=25) if n > 200 else {}   # the oracle's best iterate; its certificate is asserted
    return probs, [_reference(p, **kw) for p in probs]


def _solve(ctx, probs, **kw):
    import cmpc

    stack = [np.stack([np.asarray(p[i], float) for p in probs]) for i in range(8)]
    return cmpc.quadprog(*stack, ctx=ctx, **kw)


def _lam_of(r, k):
    return {key: v[k] for key, v in r["lambda"].items()}


def _certificate(p, x, lam):
    from oracle import qp_ipm

    H, f = p[0], p[1]
    rows, lo, hi = _stacked(p)
    y = np.hstack([lam["ineqlin"], lam["eqlin"], lam["upper"] - lam["lower"]])
    return qp_ipm.kkt_certificate(0.5 * (H + H.T), f, rows, lo, hi, x, y)


def _assert_certificate(p, x, lam, what=""):
    c = _certificate(p, x, lam)
    print(what, "certificate", c)
    assert max(c["stat_rel"], c["prim"], c["comp"], c["dual_sign"]) <= KKT_TOL, (what, c)
    return c


def _fval(p, x):
    Hs = 0.5 * (p[0] + p[0].T)
    return 0.5 * x @ Hs @ x + p[1] @ x


def _lam_dev(lam, lam_ref, weight=None):
    """Per array: |lambda - lambda_ref|_inf / max(1, |lambda_ref|_inf) (bound arrays optionally
    weighted elementwise)."""
    dev = {}
    for key in ("ineqlin", "eqlin", "lower", "upper"):
        a, b = lam[key], lam_ref[key]
        if weight is not None and key in ("lower", "upper"):
            a, b = a * weight, b * weight
        dev[key] = float(np.abs(a - b).max(initial=0.0) / max(1.0, np.abs(b).max(initial=0.0)))
    return dev


def _assert_signs(lam):
    """Inequality multipliers are >= 0 (eqlin is an equality multiplier: it has no sign)."""
    for key in ("ineqlin", "lower", "upper"):
        assert (lam[key] >= 0.0).all(), key


def _check_solution(p, ref, r, k, tol=TOL):
    """Everything test 1 asks of problem k of the result r; returns the multiplier deviations."""
    H, f, A, b, Aeq, beq, lb, ub = p
    xr, lam_ref, cert_ref, margin = ref
    x, lam = r["x"][k], _lam_of(r, k)
    assert r["exitflag"][k] == 1, r["exitflag"]
    assert np.abs(x - xr).max() < X_TOL
    fx = _fval(p, x)
    assert abs(r["fval"][k] - fx) <= 1e-9 * max(1.0, abs(fx))
    assert r["residual"][k] < tol, r["residual"][k]
    _assert_signs(lam)
    assert (lam["lower"][~np.isfinite(lb)] == 0.0).all() and (lam["upper"][~np.isfinite(ub)] == 0.0).all()
    _assert_certificate(p, x, lam, "problem %d" % k)
    assert margin >= MARGIN, margin   # a condition of the comparison below, not a skip
    dev = _lam_dev(lam, lam_ref)
    print("problem", k, "multiplier deviation", dev, "margin", margin)
    _assert_lam_dev(dev)
    return dev


# ---------------------------------------------------------------- 1, 2: multipliers and value
@pytest.mark.parametrize("seed,n,mi,me", SHAPES)
def test_multipliers_and_value_match_oracle(gpu_ctx, seed, n, mi, me):
    """n = 260 is there because every `for (i = tid; i < n; i += 256)` loop of the kernel and its
    row loops take a second trip only above 256 (two problems, oracle capped at 25 iterations)."""
    probs, refs = _family(seed, n, mi, me, 2 if n > 200 else 3)
    for ref in refs:   # a cut-short reference cannot pass silently
        c = ref[2]
        assert max(c["stat_rel"], c["prim"], c["comp"], c["dual_sign"]) <= 1e-9, c
    r = _solve(gpu_ctx, probs, tol=TOL)
    for k, (p, ref) in enumerate(zip(probs, refs)):
        _check_solution(p, ref, r, k)


def _scaled(k):
    """Problem k of the badly scaled family: x = d x', d spread over five decades."""
    rng = np.random.default_rng(200 + k)
    p = _draw(rng, 16, 12, 3)
    d = 10.0 ** rng.uniform(-2, 3, 16)
    H, f, A, b, Aeq, beq, lb, ub = p
    ps = (d[:, None] * H * d[None, :], d * f, A * d[None, :], b, Aeq * d[None, :], beq, lb / d, ub / d)
    return p, ps, d


def test_multipliers_badly_scaled_family(gpu_ctx):
    """The only place where the dsc un-scaling of x and of the bound multipliers is far from 1.
    The reference is the oracle on the unscaled problem (x' = x / d, ineqlin and eqlin unchanged,
    bound multipliers lambda' = d lambda); x and the bound multipliers are compared in the
    conditioned variable, x' d and lambda' / d."""
    cases = [_scaled(k) for k in range(4)]
    r = _solve(gpu_ctx, [c[1] for c in cases], tol=TOL)
    for k, (p, ps, d) in enumerate(cases):
        xr, lam_ref, cert_ref, margin = _reference(p)
        assert max(cert_ref.values()) <= 1e-9 and margin >= MARGIN, (cert_ref, margin)
        x, lam = r["x"][k], _lam_of(r, k)
        assert r["exitflag"][k] == 1
        assert (np.abs(x * d - xr)).max() < X_TOL
        fx = _fval(ps, x)
        assert abs(r["fval"][k] - fx) <= 1e-9 * max(1.0, abs(fx))
        assert r["residual"][k] < TOL
        _assert_signs(lam)
        assert (lam["lower"][~np.isfinite(ps[6])] == 0.0).all()
        _assert_certificate(ps, x, lam, "scaled %d" % k)
        ref_s = dict(lam_ref, lower=lam_ref["lower"] * d, upper=lam_ref["upper"] * d)
        dev = _lam_dev(lam, ref_s, weight=1.0 / d)
        print("scaled", k, "multiplier deviation", dev)
        _assert_lam_dev(dev)


# ---------------------------------------------------------------- 3: symmetric part of H
def test_symmetric_part_of_h_is_used(gpu_ctx):
    rng = np.random.default_rng(108)
    p = _draw(rng, 12, 6, 2)
    S = rng.standard_normal((12, 12))
    xr = _reference(p)[0]
    pa = (p[0] + (S - S.T),) + p[1:]
    r = _solve(gpu_ctx, [pa], tol=TOL)
    assert r["exitflag"][0] == 1
    assert np.abs(r["x"][0] - xr).max() < X_TOL
    # the other reading (x'Hx stationarity with the asymmetric matrix itself) lands far away
    from oracle import qp_ipm

    rows, lo, hi = _stacked(pa)
    assert np.abs(qp_ipm.solve_qp(pa[0], pa[1], rows, lo, hi).x - xr).max() > 1e-2


# ---------------------------------------------------------------- 4, 5: the C ABI directly
_OUTS = ("x", "fval", "exitflag", "iters", "lambda_ineqlin", "lambda_eqlin", "lambda_lower", "lambda_upper",
         "residual")


def _raw(ctx, n, mi, me, B, data, col_major=0, outs=_OUTS, fill=0.0, tol=None, max_iter=None):
    """cmpc_solve_qp_batch through ctypes: data maps cmpc_qp_data field names to arrays (absent: NULL),
    outs names the non-NULL outputs.  Returns (rc, dict of output arrays)."""
    from cmpc import _lib as L

    keep = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in data.items()}
    din = L.cmpc_qp_data(*[L.dptr(keep.get(k)) for k in ("H", "f", "A", "b", "Aeq", "beq", "lb", "ub")])
    shape = dict(x=(B, n), fval=(B,), exitflag=(B,), iters=(B,), lambda_ineqlin=(B, mi), lambda_eqlin=(B, me),
                 lambda_lower=(B, n), lambda_upper=(B, n), residual=(B,))
    o = {k: np.full(shape[k], fill, np.int32 if k in ("exitflag", "iters") else np.float64) for k in outs}
    dout = L.cmpc_qp_out(*[(L.iptr if k in ("exitflag", "iters") else L.dptr)(o.get(k)) for k in _OUTS])
    dims = L.cmpc_qp_dims(n, mi, me, B, col_major)
    rc = ctx.lib.cmpc_solve_qp_batch(ctx.h, ct.byref(dims), ct.byref(din), ct.byref(dout),
                                     ct.byref(L.opts(tol, max_iter)))
    return rc, o


def _raw_data(probs):
    return {k: np.stack([p[i] for p in probs]) for i, k in enumerate(("H", "f", "A", "b", "Aeq", "beq", "lb", "ub"))}


def test_column_major_is_bit_equal_to_row_major(gpu_ctx):
    rng = np.random.default_rng(109)
    probs = [_draw(rng, 12, 9, 3) for _ in range(3)]
    data = _raw_data(probs)
    rc, row = _raw(gpu_ctx, 12, 9, 3, 3, data)
    assert rc == 0 and (row["exitflag"] == 1).all()
    cm = dict(data, A=np.ascontiguousarray(data["A"].transpose(0, 2, 1)),
              Aeq=np.ascontiguousarray(data["Aeq"].transpose(0, 2, 1)))
    rc, col = _raw(gpu_ctx, 12, 9, 3, 3, cm, col_major=1)
    assert rc == 0
    for k in _OUTS:
        assert np.array_equal(row[k], col[k]), k
    # and the row-major call is the one cmpc.quadprog makes
    assert np.array_equal(row["x"], _solve(gpu_ctx, probs)["x"])


def test_optional_outputs_and_arguments(gpu_ctx):
    rng = np.random.default_rng(110)
    probs = [_draw(rng, 12, 9, 3) for _ in range(2)]
    data = _raw_data(probs)
    rc, full = _raw(gpu_ctx, 12, 9, 3, 2, data)
    assert rc == 0 and (full["exitflag"] == 1).all()
    rc, only_x = _raw(gpu_ctx, 12, 9, 3, 2, data, outs=("x",))
    assert rc == 0 and np.array_equal(only_x["x"], full["x"])
    for k in _OUTS[1:]:
        rc, o = _raw(gpu_ctx, 12, 9, 3, 2, data, outs=("x", k), fill=-77)
        assert rc == 0 and np.array_equal(o["x"], full["x"]), k
        assert np.array_equal(o[k], full[k]), k

    def drop(*names):
        return {k: v for k, v in data.items() if k not in names}

    # an absent argument is the full call with that part written out as what the contract says is
    # inactive: infinite bounds, all-zero rows that can hold (dropped)
    inf = np.full((2, 12), np.inf)
    written = {("ub",): dict(ub=inf), ("lb",): dict(lb=-inf),
               ("Aeq", "beq"): dict(Aeq=np.zeros((2, 3, 12)), beq=np.zeros((2, 3))),
               ("A", "b"): dict(A=np.zeros((2, 9, 12)), b=np.ones((2, 9)))}
    keys = ("H", "f", "A", "b", "Aeq", "beq", "lb", "ub")
    for absent, explicit in written.items():
        mi, me = (0 if "A" in absent else 9), (0 if "Aeq" in absent else 3)
        rc, o = _raw(gpu_ctx, 12, mi, me, 2, drop(*absent))
        assert rc == 0 and (o["exitflag"] == 1).all(), absent
        rc, e = _raw(gpu_ctx, 12, 9, 3, 2, dict(data, **explicit))
        assert rc == 0 and np.array_equal(o["x"], e["x"]), absent
        for k in ("fval", "exitflag", "iters", "lambda_lower", "lambda_upper", "residual"):
            assert np.array_equal(o[k], e[k]), (absent, k)
        # and it is that problem's optimum
        for j in range(2):
            p = tuple(explicit[key][j] if key in explicit else data[key][j] for key in keys)
            assert np.abs(o["x"][j] - _reference(p)[0]).max() < X_TOL, absent


def test_api_errors(gpu_ctx):
    from cmpc import _lib as L

    one = np.zeros(1)

    def err(rc, code):
        msg = gpu_ctx.lib.cmpc_last_error(gpu_ctx.h)
        assert rc == code and msg, (rc, msg)

    rc, _ = _raw(gpu_ctx, 0, 0, 0, 1, dict(H=one, f=one), outs=())
    err(rc, L.CMPC_ERR_ARG)      # out->x NULL
    x = np.zeros(4)
    dout = L.cmpc_qp_out(L.dptr(x), *[None] * 8)

    def call(n, mi, me, B, **data):
        din = L.cmpc_qp_data(*[L.dptr(data.get(k)) for k in ("H", "f", "A", "b", "Aeq", "beq", "lb", "ub")])
        dims = L.cmpc_qp_dims(n, mi, me, B, 0)
        return gpu_ctx.lib.cmpc_solve_qp_batch(gpu_ctx.h, ct.byref(dims), ct.byref(din), ct.byref(dout), None)

    err(call(0, 0, 0, 1, H=one, f=one), L.CMPC_ERR_ARG)
    err(call(2, 1, 0, 1, H=np.eye(2), f=np.zeros(2), b=one), L.CMPC_ERR_ARG)
    err(call(2, 0, 1, 1, H=np.eye(2), f=np.zeros(2), Aeq=np.ones((1, 2))), L.CMPC_ERR_ARG)
    # checked before anything is allocated or read: the pointers are tiny dummies
    err(call(15000, 0, 0, 1, H=one, f=one), L.CMPC_ERR_UNSUPPORTED)
    x[:] = -77.0
    assert call(2, 0, 0, 0, H=np.eye(2), f=np.zeros(2)) == L.CMPC_OK
    assert (x == -77.0).all()


# ---------------------------------------------------------------- 6: isolation in a mixed batch
def test_mixed_batch_isolation(gpu_ctx):
    rng = np.random.default_rng(111)
    probs = [list(_draw(rng, 8, 6, 2)) for _ in range(6)]
    probs[2][6], probs[2][7] = probs[2][6].copy(), probs[2][7].copy()
    probs[2][6][0], probs[2][7][0] = 1.0, 0.5                                   # crossed bounds
    probs[3][0], probs[3][6], probs[3][7] = -np.eye(8), -np.ones(8), np.ones(8)  # concave inside a box
    probs[4][1] = probs[4][1].copy()
    probs[4][1][3] = np.nan                                                      # NaN in f
    probs[5][2], probs[5][3] = probs[5][2].copy(), probs[5][3].copy()
    probs[5][2][1], probs[5][3][1] = 0.0, 1.0                                    # 0 x <= 1: dropped
    probs = [tuple(p) for p in probs]
    good = [0, 1, 5]
    r = _solve(gpu_ctx, probs)
    flag = r["exitflag"]
    assert list(flag[:4]) == [1, 1, -2, -6] and flag[4] != 1 and flag[5] == 1, flag
    assert r["lambda"]["ineqlin"][5][1] == 0.0
    assert np.abs(r["x"][5] - _reference(probs[5])[0]).max() < X_TOL

    def fields(res, k):
        return [res["x"][k], res["fval"][k], res["exitflag"][k], res["iterations"][k], res["residual"][k]] + \
               [res["lambda"][key][k] for key in ("ineqlin", "eqlin", "lower", "upper")]

    for k in good:
        alone = _solve(gpu_ctx, [probs[k]])
        for a, c in zip(fields(r, k), fields(alone, 0)):
            assert np.all(np.isfinite(a)) and np.array_equal(a, c), k
    rev = _solve(gpu_ctx, probs[::-1])
    for k in range(6):
        for a, c in zip(fields(r, k), fields(rev, 5 - k)):
            assert np.array_equal(a, c, equal_nan=True), k


# ---------------------------------------------------------------- 7: exit flags
def test_flag_minus_infinity_bounds_are_infeasible(gpu_ctx):
    """b_r = -inf, ub_i = -inf and lb_i = +inf admit no point: -2, not a dropped row."""
    import cmpc

    p = _family(2, 8, 6, 2, 3)[0][0]
    for i, v in [(3, -np.inf), (7, -np.inf), (6, np.inf)]:
        q = [a.copy() for a in p]
        q[i][2] = v
        r = cmpc.quadprog(*q, ctx=gpu_ctx)
        assert r["exitflag"] == -2, (i, r["exitflag"])
    # +inf on the harmless side stays an absent bound
    q = [a.copy() for a in p]
    q[3][2], q[7][2], q[6][1] = np.inf, np.inf, -np.inf
    assert cmpc.quadprog(*q, ctx=gpu_ctx)["exitflag"] == 1


def test_flag_unbounded(gpu_ctx):
    import cmpc

    r = cmpc.quadprog(np.zeros((1, 1)), -np.ones(1), ctx=gpu_ctx)
    assert r["exitflag"] == -3
    r = cmpc.quadprog(np.diag([1.0, 0.0]), np.array([0.0, -1.0]), lb=np.zeros(2), ctx=gpu_ctx)
    assert r["exitflag"] == -3


def test_flag_iteration_cap(gpu_ctx):
    """A healthy solve cut off by MaxIterations reports 0 (CMPC_QP_MAXITER), not infeasible or
    unbounded; the same problems at the default cap give 1."""
    probs, refs = _family(3, 20, 15, 5, 3)
    r = _solve(gpu_ctx, probs, max_iter=3)
    assert (r["exitflag"] == 0).all(), r["exitflag"]
    assert (r["iterations"] == 3).all()
    assert np.isfinite(r["x"]).all()
    for k, p in enumerate(probs):
        fx = _fval(p, r["x"][k])
        assert abs(r["fval"][k] - fx) <= 1e-9 * max(1.0, abs(fx))
    assert (_solve(gpu_ctx, probs)["exitflag"] == 1).all()
    # a box-only problem starts primal feasible: the cap is still 0, not "unbounded"
    box = [(p[0], p[1], p[2][:0], p[3][:0], p[4][:0], p[5][:0], np.full(20, -2.0), np.full(20, 2.0)) for p in probs]
    r = _solve(gpu_ctx, box, max_iter=3)
    assert (r["exitflag"] == 0).all() and (r["iterations"] == 3).all(), r["exitflag"]


def test_flag_semidefinite_but_bounded(gpu_ctx):
    rng = np.random.default_rng(107)
    n = 10
    H = np.diag([1.0, 1.0, 1.0] + [0.0] * (n - 3))
    f = rng.standard_normal(n)
    e = np.zeros((0, n))
    p = (H, f, e, np.zeros(0), e, np.zeros(0), -np.ones(n), np.ones(n))
    ref = _reference(p)
    assert ref[3] >= MARGIN, ref[3]
    r = _solve(gpu_ctx, [p], tol=TOL)
    _check_solution(p, ref, r, 0)
    assert np.abs(r["x"][0][3:] + np.sign(f[3:])).max() < X_TOL


# ---------------------------------------------------------------- 8: fixed variables
def test_fixed_variables(gpu_ctx):
    """lb_i == ub_i (MATLAB callers pass it routinely) pins x_i.  Both bound rows of such a variable
    are active at every feasible point, so its two bound multipliers are not unique: only upper - lower,
    its equality multiplier, is compared (for the other variables the arrays themselves)."""
    rng = np.random.default_rng(112)
    probs = []
    for _ in range(2):
        p = list(_draw(rng, 12, 6, 2))
        p[6][4] = p[7][4] = 0.3
        p[6][7] = p[7][7] = -0.1
        probs.append(tuple(p))
    r = _solve(gpu_ctx, probs, tol=TOL)
    for k, p in enumerate(probs):
        xr, lam_ref, cert_ref, margin = _reference(p)
        assert max(cert_ref.values()) <= 1e-9, cert_ref
        x, lam = r["x"][k], _lam_of(r, k)
        assert r["exitflag"][k] == 1, r["exitflag"]
        assert abs(x[4] - 0.3) <= 1e-9 and abs(x[7] + 0.1) <= 1e-9, (x[4], x[7])
        assert np.abs(x - xr).max() < X_TOL
        _assert_signs(lam)
        assert (lam["lower"][~np.isfinite(p[6])] == 0.0).all()
        _assert_certificate(p, x, lam, "fixed %d" % k)
        assert margin >= MARGIN, margin
        fixed = p[6] == p[7]
        diff, diff_ref = lam["upper"] - lam["lower"], lam_ref["upper"] - lam_ref["lower"]
        dev = _lam_dev({key: np.where(fixed, 0.0, v) if key in ("lower", "upper") else v for key, v in lam.items()},
                       {key: np.where(fixed, 0.0, v) if key in ("lower", "upper") else v for key, v in lam_ref.items()})
        dev["fixed"] = float(np.abs(diff - diff_ref)[fixed].max() / max(1.0, np.abs(diff_ref[fixed]).max()))
        print("fixed", k, "multiplier deviation", dev)
        _assert_lam_dev(dev)
        assert dev["fixed"] < LAM_TOL["upper"], dev   # measured 1.9e-9


# ---------------------------------------------------------------- 9: multipliers of the returned point
def test_multipliers_belong_to_returned_point_on_stalled_exit(gpu_ctx):
    """tol = 1e-13 is below the rounding floor: the solve ends stalled and returns its best iterate.
    x and lambda must be that iterate's, so the complementarity of the returned pair is no worse
    than 10x the one of the tol = 1e-9 solve.  Measured on an MI355X, per problem, comp at
    tol = 1e-13 / at tol = 1e-9: 6.2e-14 / 2.5e-9, 1.1e-9 / 1.1e-9 (the best iterate of the tight solve is
    the one the loose solve stopped at), 5.7e-13 / 2.3e-8.  The parent kernel passes this too: on a
    stalled exit its last iterate's multipliers are within rounding of the best iterate's.  The
    mismatch shows on a cap exit, test_multipliers_belong_to_returned_point_on_cap_exit."""
    probs, refs = _family(4, 40, 30, 0, 3)
    tight = _solve(gpu_ctx, probs, tol=1e-13)
    loose = _solve(gpu_ctx, probs, tol=1e-9)
    assert (tight["exitflag"] == 1).all() and (loose["exitflag"] == 1).all()
    for k, p in enumerate(probs):
        ct_ = _assert_certificate(p, tight["x"][k], _lam_of(tight, k), "tol 1e-13, %d" % k)
        cl_ = _assert_certificate(p, loose["x"][k], _lam_of(loose, k), "tol 1e-9, %d" % k)
        print("problem", k, "comp at 1e-13", ct_["comp"], "at 1e-9", cl_["comp"], "residual", tight["residual"][k],
              loose["residual"][k], "iterations", tight["iterations"][k], loose["iterations"][k])
        assert ct_["comp"] <= 10.0 * cl_["comp"], (ct_, cl_)
        assert np.abs(tight["x"][k] - refs[k][0]).max() < X_TOL
        assert tight["residual"][k] <= loose["residual"][k]


def test_multipliers_belong_to_returned_point_on_cap_exit(gpu_ctx):
    """A solve cut off by the cap returns its best iterate, whose merit is `residual`.  The same solve
    with a tolerance just above that merit converges at that very iterate and returns it: x and every
    multiplier array of the two must be the same bits."""
    probs, _ = _family(4, 40, 30, 0, 3)
    for k, p in enumerate(probs):
        cut = _solve(gpu_ctx, [p], tol=1e-13, max_iter=6)
        assert cut["exitflag"][0] == 0 and cut["iterations"][0] == 6
        conv = _solve(gpu_ctx, [p], tol=cut["residual"][0] * (1.0 + 1e-9), max_iter=6)
        assert conv["exitflag"][0] == 1 and conv["residual"][0] == cut["residual"][0]
        assert np.array_equal(cut["x"], conv["x"]) and cut["fval"][0] == conv["fval"][0]
        for key in ("ineqlin", "lower", "upper"):
            assert np.array_equal(cut["lambda"][key], conv["lambda"][key]), (k, key)
