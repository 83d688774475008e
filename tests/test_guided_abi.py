"""CPU: the depth refinement's entry points (mi_depth_guided*, mi_stack_depth_map_refined*, mi_dmap_depth_map_refined*) are
declared, exported and bound, and every argument check returns MI_ERR_INVALID with the argument named, before any device call
and before the handle is looked at -- the handle forms are called with a null handle and with a block of zeros in its place."""
import ctypes
import re

import numpy as np
import pytest

from test_abi import HEADER, header_symbols

NAMES = {"mi_depth_guided": 13, "mi_depth_guided_device": 15, "mi_stack_depth_map_refined": 7, "mi_stack_depth_map_refined_device": 7,
         "mi_dmap_depth_map_refined": 7, "mi_dmap_depth_map_refined_device": 7}
H, W = 4, 6


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from shinestacker_amd import depth_out
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name, n in NAMES.items():
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
        assert len(hiplib.SIGNATURES[name][1]) == n, name
    text = open(HEADER).read()
    assert re.search(r"#define MI_ABI_VERSION 1\b", text) and hiplib.load().mi_abi_version() == 1
    assert re.search(r"MI_GUIDED_SCRATCH_PLANES = 7\b", text) and depth_out.SCRATCH_PLANES == 7
    assert re.search(r"MI_GUIDED_MAX_RADIUS = 32\b", text) and depth_out.MAX_REFINE_RADIUS == 32


@pytest.fixture()
def planes():
    return {"p": np.zeros((H, W), np.float32), "w": np.ones((H, W), np.float64), "g": np.zeros((H, W, 3), np.uint16),
            "out": np.zeros((H, W), np.float32), "scratch": np.zeros((7 * H * W + 2,), np.float64)}


def expect(hiplib, rc, msg):
    err = hiplib.load().mi_last_error()
    assert rc == hiplib.MI_ERR_INVALID and msg in err, (msg, rc, err)


@pytest.mark.parametrize("form", ["host", "device"])
def test_plane_forms_check_every_argument(hiplib, planes, form):
    lib = hiplib.load()
    U8, U16, F32, F64 = hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32, hiplib.MI_F64
    sc = planes["scratch"].ctypes.data
    sc += -sc % 16
    base = dict(v=planes["p"].ctypes.data, w=planes["w"].ctypes.data, wt=F64, g=planes["g"].ctypes.data, gt=U16, h=H, wd=W, r=6, eps=1e-4,
                lo=0.0, hi=5.0, out=planes["out"].ctypes.data, scratch=sc)

    def call(**kw):
        a = dict(base, **kw)
        if form == "host":
            return lib.mi_depth_guided(0, a["v"], a["w"], a["wt"], a["g"], a["gt"], a["h"], a["wd"], a["r"], a["eps"], a["lo"], a["hi"],
                                       a["out"])
        return lib.mi_depth_guided_device(0, None, a["v"], a["w"], a["wt"], a["g"], a["gt"], a["h"], a["wd"], a["r"], a["eps"], a["lo"],
                                          a["hi"], a["scratch"], a["out"])
    expect(hiplib, call(v=None), b"value is null")
    expect(hiplib, call(w=None), b"weight is null")
    expect(hiplib, call(g=None), b"guide is null")
    expect(hiplib, call(out=None), b"out is null")
    for h in (0, -3):
        expect(hiplib, call(h=h), b"height must be at least 1")
        expect(hiplib, call(wd=h), b"width must be at least 1")
    expect(hiplib, call(h=40000, wd=40000), b"too large")
    for r in (0, -1, 33, 1 << 20):
        expect(hiplib, call(r=r), b"radius must be in [1, 32]")
    for eps in (0.0, 9.9e-10, 1000.0001, -1e-4, float("nan"), float("inf")):
        expect(hiplib, call(eps=eps), b"eps must be in [1e-9, 1e3]")
    expect(hiplib, call(lo=5.5), b"lo must not exceed hi")
    for bad in (float("nan"), float("inf"), -float("inf")):
        expect(hiplib, call(lo=bad), b"lo and hi must be finite")
        expect(hiplib, call(hi=bad), b"lo and hi must be finite")
    for gt in (F32, F64, 7, -1):
        expect(hiplib, call(gt=gt), b"guide_dtype must be MI_U8 or MI_U16")
    for wt in (U8, U16, 9):
        expect(hiplib, call(wt=wt), b"weight_float_type must be MI_F32 or MI_F64")
    if form == "device":
        expect(hiplib, call(scratch=None), b"scratch is null")
        expect(hiplib, call(scratch=sc + 8), b"scratch is not aligned")
        expect(hiplib, call(v=base["v"] + 2), b"value and out are float32 planes")
        expect(hiplib, call(out=base["out"] + 1), b"value and out are float32 planes")
        expect(hiplib, call(w=base["w"] + 4), b"weight is not aligned")
        expect(hiplib, call(g=base["g"] + 1), b"guide is not aligned")


@pytest.mark.parametrize("name", [n for n in NAMES if "refined" in n])
def test_handle_forms_check_every_argument(hiplib, planes, name):
    lib = hiplib.load()
    fn = getattr(lib, name)
    g, out = planes["g"].ctypes.data, planes["out"].ctypes.data
    U8, U16 = hiplib.MI_U8, hiplib.MI_U16
    expect(hiplib, fn(None, 0.0, g, U16, 6, 1e-4, out), b"null handle")
    expect(hiplib, fn(None, 0.0, None, 99, 0, 0.0, None), b"null handle")
    zeros = np.zeros(1 << 16, np.uint8)         # stands where a handle would: the checks below come before it is read
    h = zeros.ctypes.data
    expect(hiplib, fn(h, 0.0, None, U16, 6, 1e-4, out), b"guide is null")
    expect(hiplib, fn(h, 0.0, g, U16, 6, 1e-4, None), b"out is null")
    for gt in (hiplib.MI_F32, hiplib.MI_F64, 5):
        expect(hiplib, fn(h, 0.0, g, gt, 6, 1e-4, out), b"guide_dtype must be MI_U8 or MI_U16")
    for r in (0, 33, -6):
        expect(hiplib, fn(h, 0.0, g, U8, r, 1e-4, out), b"radius must be in [1, 32]")
    for eps in (0.0, 1e-10, 1e4, float("nan"), float("inf")):
        expect(hiplib, fn(h, 0.0, g, U8, 6, eps, out), b"eps must be in [1e-9, 1e3]")
    if name.endswith("_device"):
        expect(hiplib, fn(h, 0.0, g + 1, U16, 6, 1e-4, out), b"guide is not aligned")
    assert not zeros.any()
