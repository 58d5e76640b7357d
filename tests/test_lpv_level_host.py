"""The reference structure of a structured batch on the host (include/cmpc.h, cmpc_mpc_lpv_level): the numpy
statement cmpc.structure.lpv_level on the reference's own QPs and on batches that must not qualify, and the
header's two flags.  No GPU."""
import re

import numpy as np
import pytest

from conftest import LPV_CASES
from lpv_level_cases import PLANTS, copy_of, plant, recognised, stacked

CONDENSED = [n for n in LPV_CASES if n != "lpv_n125_a3"]


@pytest.mark.parametrize("name", LPV_CASES)
def test_captured_qps_hold_the_pattern_at_level_2(name):
    """Every captured QP of every golden file, through structure.recognize, holds the pattern with Q zero on states
    1, 2, 5, 6.  The five condensed files are eligible: level 2.  lpv_n125_a3 holds the same pattern (conforms, Q at
    level 2) but its horizon is beyond the condensed kernels (N = 125 > 32), so by the definition its level is 0."""
    from cmpc import structure as St

    for c, p in recognised(name):
        assert St.lpv_conforms(p).all()
        Q = np.asarray(p["Q"])
        assert np.array_equal(Q, np.diag([10.0, 0, 0, 25.0, 10.0, 0, 0, 0, 0]))
        assert np.array_equal(p["row_slack"], [-1, 0, 1, 1, 2, 2, 2][: p["mc"]])
        assert np.array_equal(p["row_sign"], [1, 1, 1, 1, -1, -1, -1][: p["mc"]])
        lv = St.lpv_level(p)
        assert lv.dtype == np.int32 and lv.shape == (1,)
        if name in CONDENSED:
            assert St.lpv_eligible(p) == 2 and lv[0] == 2, (name, lv)
        else:
            assert p["N"] == 125 and St.lpv_eligible(p) == 0 and lv[0] == 0
            short = dict(p, N=30, **{k: p[k][:, :30] for k in ("A", "B", "C", "h")}, qlin=p["qlin"][:, :31])
            assert St.lpv_level(short)[0] == 2       # the same data at a condensed horizon


def test_level_1_and_the_ineligible_batches():
    from cmpc import structure as St

    p = stacked("lpv_n20_a4")
    B = p["A"].shape[0]
    assert p["mc"] == 7 and (St.lpv_level(p) == 2).all()
    q = copy_of(p)
    q["Q"][1, 1] = 3.0
    assert (St.lpv_level(q) == 1).all()
    q = copy_of(p)
    q["Q"][0, 3] = 1e-300                                    # an off-diagonal Q entry
    assert (St.lpv_level(q) == 0).all() and St.lpv_level(q).shape == (B,)
    q = copy_of(p)
    q["row_slack"] = np.asarray(p["row_slack"])[[0, 2, 1, 3, 4, 5, 6]].copy()   # {-1, 1, 0, 1, 2, 2, 2}
    assert (St.lpv_level(q) == 0).all()
    q = copy_of(p)
    q["row_sign"] = -np.asarray(p["row_sign"])
    assert (St.lpv_level(q) == 0).all()
    # nb = 4: one more plane row
    q = copy_of(p)
    q["mc"] = 8
    q["row_slack"] = np.r_[p["row_slack"], 2].astype(np.int32)
    q["row_sign"] = np.r_[p["row_sign"], -1].astype(np.int32)
    q["C"] = np.concatenate([p["C"], p["C"][:, :, -1:]], axis=2)
    q["h"] = np.concatenate([p["h"], p["h"][:, :, -1:]], axis=2)
    assert St.lpv_conforms(q).all() and (St.lpv_level(q) == 0).all()
    # nx = 4: a double-integrator-shaped dict with the v3 row tables
    rng = np.random.default_rng(0)
    di = dict(nx=4, nu=2, N=9, ns=3, mc=6, Q=np.eye(4), R=np.eye(2), dR=np.eye(2), Qs=np.ones(3), u_ub=np.ones(2),
              u_lb=-np.ones(2), row_slack=np.array([-1, 0, 1, 1, 2, 2], np.int32),
              row_sign=np.array([1, 1, 1, 1, -1, -1], np.int32), A=np.tile(np.eye(4), (3, 9, 1, 1)),
              B=np.zeros((3, 9, 4, 2)), x0=np.zeros((3, 4)), u_prev=np.zeros((3, 2)), qlin=np.zeros((3, 10, 4)),
              C=rng.standard_normal((3, 9, 6, 4)), h=np.ones((3, 9, 6)))
    assert np.array_equal(St.lpv_level(di), np.zeros(3, np.int32))


def test_plants_lower_exactly_their_agent():
    """Each planted violation takes its agent, and only it, to level 0; -0.0 in a slot that must be zero does not."""
    from cmpc import structure as St

    p = stacked("lpv_n20_a4")
    B, N = p["A"].shape[0], p["N"]
    for which in range(len(PLANTS)):
        for a, k in ((0, 0), (B - 1, N - 1)):
            q = copy_of(p)
            plant(q, a, which, k)
            want = np.full(B, 2, np.int32)
            want[a] = 0
            assert np.array_equal(St.lpv_level(q), want), PLANTS[which]
    q = copy_of(p)
    q["A"][:, :, 5, 4] = -0.0
    q["B"][:, :, 7, 1] = -0.0
    q["C"][:, :, 1, 8] = -0.0
    assert (St.lpv_level(q) == 2).all()


def test_header_flags_and_abi():
    from cmpc import _lib as L

    src = open(L.HEADER).read()
    m1 = re.search(r"#define\s+CMPC_FLAG_LPV\s+(\d+)\b", src)
    m2 = re.search(r"#define\s+CMPC_FLAG_LPV_AUTO\s+(\d+)\b", src)
    assert m1 and m2
    f1, f2 = int(m1.group(1)), int(m2.group(1))
    assert (f1, f2) == (16384, 32768) == (L.CMPC_FLAG_LPV, L.CMPC_FLAG_LPV_AUTO)
    # distinct single bits, distinct from every other flag of the header
    others = {n: int(v) for n, v in re.findall(r"#define\s+(CMPC_FLAG_(?!ALL|LPV)\w+)\s+(\d+)\b", src)}
    assert len(others) >= 12
    for f in (f1, f2):
        assert f & (f - 1) == 0 and all(not (f & v) for v in others.values()), others
    assert f1 != f2
    all_ = re.search(r"#define\s+CMPC_FLAG_ALL\s+\((.*?)\)", src, flags=re.S).group(1)
    names = set(re.findall(r"CMPC_FLAG_\w+", all_))
    assert {"CMPC_FLAG_LPV", "CMPC_FLAG_LPV_AUTO"} <= names and set(others) <= names
    assert re.search(r"#define\s+CMPC_ABI_VERSION\s+6\b", src)       # additions only
    for fn in ("cmpc_mpc_lpv_level", "cmpc_mpc_lpv_level_dev"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", src) and fn in L.SIGNATURES
    assert L.lpv_flags(False) == 0 and L.lpv_flags(True) == f1 and L.lpv_flags("auto") == f2
    with pytest.raises(ValueError):
        L.lpv_flags("always")
