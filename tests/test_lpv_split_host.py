"""CMPC_FLAG_LPV_SPLIT and cmpc_mpc_lpv_split_dev without a device (include/cmpc.h): the flag's bit and its place in
the header, the new entry in the header, the built library and the bindings, what cmpc_plan_mpc reports under the
flag, and the numpy statement of the partition (cmpc.structure.lpv_split)."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "cmpc.h")


def _defines():
    """{name: literal value} of the header's #define lines with an integer literal."""
    out = {}
    with open(HEADER) as f:
        for m in re.finditer(r"^#define\s+(CMPC_\w+)\s+\(?(-?\d+)\)?\s", f.read(), re.M):
            out[m.group(1)] = int(m.group(2))
    return out


def test_the_flag_in_the_header():
    d = _defines()
    assert d["CMPC_FLAG_LPV_SPLIT"] == 65536
    assert d["CMPC_ABI_VERSION"] == 6
    flags = {k: v for k, v in d.items() if k.startswith("CMPC_FLAG_")}
    assert bin(flags["CMPC_FLAG_LPV_SPLIT"]).count("1") == 1
    for k, v in flags.items():
        if k != "CMPC_FLAG_LPV_SPLIT":
            assert v & 65536 == 0, k
    text = open(HEADER).read()
    m = re.search(r"#define\s+CMPC_FLAG_ALL\s+\(((?:[^)\\]|\\\n)*)\)", text)
    assert m, "CMPC_FLAG_ALL"
    listed = set(re.findall(r"CMPC_FLAG_\w+", m.group(1)))
    assert "CMPC_FLAG_LPV_SPLIT" in listed
    assert listed == set(flags), listed ^ set(flags)


def test_the_flag_and_the_entry_in_the_bindings():
    from cmpc import _lib as L

    assert L.CMPC_FLAG_LPV_SPLIT == 65536
    assert L.lpv_flags("split") == 65536
    assert L.lpv_flags("auto") == 32768 and L.lpv_flags(True) == 16384 and L.lpv_flags(False) == 0
    with pytest.raises(ValueError):
        L.lpv_flags("always")
    assert re.search(r"\bint\s+cmpc_mpc_lpv_split_dev\s*\(", open(HEADER).read())
    res, args = L.SIGNATURES["cmpc_mpc_lpv_split_dev"]
    assert res is ct.c_int and len(args) == 6 and args[1] is ct.c_int
    lib = L.load()
    assert lib.cmpc_abi_version() == 6
    assert hasattr(lib, "cmpc_mpc_lpv_split_dev")       # exported by the built library


def _plan(p, flags):
    from cmpc import _lib as L
    from cmpc.solver import _dims, _weights

    w, keep = _weights(p)
    info = L.cmpc_plan_info()
    o = L.opts(None, None, flags)
    rc = L.load().cmpc_plan_mpc(ct.byref(_dims(p, 4)), ct.byref(w), ct.byref(o), ct.byref(info))
    del keep
    return rc, tuple(getattr(info, f) for f, _ in info._fields_)


def test_the_plan_reports_the_general_image_under_the_flag():
    from cmpc import _lib as L
    from lpv_level_cases import stacked

    p = stacked("lpv_n10_a2")
    base = L.CMPC_FLAG_RESCUE | L.CMPC_FLAG_POLISH
    rc0, plain = _plan(p, base)
    rc1, split = _plan(p, base | 65536)
    rc2, both = _plan(p, base | 65536 | 16384)
    rc3, promise = _plan(p, base | 16384)
    assert rc0 == rc1 == rc2 == rc3 == L.CMPC_OK
    assert split == plain
    assert both == promise and both != plain
    lds = [f for f, _ in L.cmpc_plan_info._fields_].index("lds_bytes")
    assert both[lds] < plain[lds]
    assert _plan(p, 65536)[1] == _plan(p, 0)[1]
    assert _plan(p, 131072)[0] == L.CMPC_ERR_ARG       # the next bit is still nobody's


def _check_split(level):
    from cmpc import structure as St

    level = np.asarray(level, np.int32)
    batch = level.size
    conf, rest = St.lpv_split(level)
    assert conf.dtype == rest.dtype == np.int32 and conf.shape == rest.shape == (batch + 1,)
    nc, nr = int(conf[batch]), int(rest[batch])
    assert nc + nr == batch and nc == int((level > 0).sum())
    a, b = conf[:nc], rest[:nr]
    assert (np.diff(a) > 0).all() and (np.diff(b) > 0).all()        # ascending
    assert not set(a.tolist()) & set(b.tolist())                    # disjoint
    assert sorted(a.tolist() + b.tolist()) == list(range(batch))    # together every agent
    assert (level[a] > 0).all() and (level[b] <= 0).all()
    assert (conf[nc:batch] == -1).all() and (rest[nr:batch] == -1).all()
    return conf, rest


def test_the_numpy_statement_of_the_partition():
    conf, rest = _check_split([])                                   # batch 0: the two counts alone
    assert conf.tolist() == [0] and rest.tolist() == [0]
    conf, rest = _check_split([2])
    assert conf.tolist() == [0, 1] and rest.tolist() == [-1, 0]
    conf, rest = _check_split([0])
    assert conf.tolist() == [-1, 0] and rest.tolist() == [0, 1]
    conf, rest = _check_split([1, 2, 2, 1, 1])                      # all conforming (level 2 counts)
    assert conf.tolist() == [0, 1, 2, 3, 4, 5] and rest.tolist() == [-1] * 5 + [0]
    conf, rest = _check_split([0] * 5)                              # none
    assert rest.tolist() == [0, 1, 2, 3, 4, 5] and conf.tolist() == [-1] * 5 + [0]
    conf, rest = _check_split([0, 2, 0, 1, 2, 0, 0])
    assert conf.tolist() == [1, 3, 4, -1, -1, -1, -1, 3] and rest.tolist() == [0, 2, 5, 6, -1, -1, -1, 4]
    rng = np.random.default_rng(5)
    for batch in (63, 64, 65, 1025):
        _check_split(rng.integers(0, 3, batch))
