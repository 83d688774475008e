"""CPU: the feature estimator's C boundary -- mi_feat_* declared in include/mi355stack.h, exported by the library, bound in
_lib.SIGNATURES with as many arguments as the header gives them, and every argument check answered with MI_ERR_INVALID and the
argument's name before any device call (no GPU is needed to be refused)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["mi_feat_gray", "mi_feat_score", "mi_feat_extract", "mi_feat_match", "mi_feat_ransac"]
U8, U16, F32 = 0, 1, 2


def _header():
    text = open(os.path.join(ROOT, "include", "mi355stack.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("base", NAMES)
def test_declared_exported_and_bound(hiplib, base):
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    text = _header()
    for name in (base, base + "_device"):
        m = re.search(rf"MI_API int {name}\((.*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in hiplib.SIGNATURES
        assert len(hiplib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    # the device form takes the stream after the device and otherwise the same arguments
    assert len(hiplib.SIGNATURES[base + "_device"][1]) == len(hiplib.SIGNATURES[base][1]) + 1


def test_dtype_codes(hiplib):
    assert (hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32) == (U8, U16, F32)


def refused(hiplib, rc, text):
    assert rc == hiplib.MI_ERR_INVALID
    assert text in hiplib.load().mi_last_error().decode(), hiplib.load().mi_last_error()


def test_gray_checks(hiplib):
    lib = hiplib.load()
    a = np.zeros((8, 8, 3), np.uint8)
    o = np.zeros((8, 8), np.uint8)
    p, q = a.ctypes.data, o.ctypes.data
    for dev in (False, True):
        f = (lambda *x: lib.mi_feat_gray_device(0, None, *x)) if dev else (lambda *x: lib.mi_feat_gray(0, *x))
        refused(hiplib, f(None, 8, 8, 3, U8, q), "null frame")
        refused(hiplib, f(p, 0, 8, 3, U8, q), "height and width must be >= 1")
        refused(hiplib, f(p, 8, -1, 3, U8, q), "height and width must be >= 1")
        refused(hiplib, f(p, 32769, 8, 3, U8, q), "must be <= 32768")
        refused(hiplib, f(p, 8, 8, 2, U8, q), "channels must be 1 or 3")
        refused(hiplib, f(p, 8, 8, 3, F32, q), "dtype must be MI_U8 or MI_U16")
        refused(hiplib, f(p, 8, 8, 3, U8, None), "null gray plane")


def test_score_checks(hiplib):
    lib = hiplib.load()
    g = np.zeros((40, 40), np.uint8)
    s = np.zeros((40, 40), np.uint8)
    h = np.zeros(256, np.uint32)
    p, q, r = g.ctypes.data, s.ctypes.data, h.ctypes.data
    for dev in (False, True):
        f = (lambda *x: lib.mi_feat_score_device(0, None, *x)) if dev else (lambda *x: lib.mi_feat_score(0, *x))
        refused(hiplib, f(None, 40, 40, 20, q, r), "null gray plane")
        refused(hiplib, f(p, 0, 40, 20, q, r), "height and width must be >= 1")
        refused(hiplib, f(p, 40, 40000, 20, q, r), "must be <= 32768")
        refused(hiplib, f(p, 40, 40, -1, q, r), "threshold must be in [0, 254]")
        refused(hiplib, f(p, 40, 40, 255, q, r), "threshold must be in [0, 254]")
        refused(hiplib, f(p, 40, 40, 20, None, r), "null score plane")
        refused(hiplib, f(p, 40, 40, 20, q, None), "null histogram")


def test_extract_checks(hiplib):
    from shinestacker_amd import features as ft
    lib = hiplib.load()
    a = np.zeros((40, 40, 3), np.uint8)
    kp = np.zeros((3500, 5), np.int32)
    de = np.zeros((3500, 32), np.uint8)
    n = ctypes.c_int(-7)
    pat = np.array(ft.pattern())
    p, t, k, d, nn = a.ctypes.data, pat.ctypes.data, kp.ctypes.data, de.ctypes.data, ctypes.byref(n)
    far = pat.copy()
    far[31, 255, 3] = 14
    for dev in (False, True):
        f = (lambda *x: lib.mi_feat_extract_device(0, None, *x)) if dev else (lambda *x: lib.mi_feat_extract(0, *x))
        refused(hiplib, f(None, 40, 40, 3, U8, 3, 2000, 20, t, 3500, k, d, nn), "null frame")
        refused(hiplib, f(p, 0, 40, 3, U8, 3, 2000, 20, t, 3500, k, d, nn), "height and width must be >= 1")
        refused(hiplib, f(p, 40, 40, 4, U8, 3, 2000, 20, t, 3500, k, d, nn), "channels must be 1 or 3")
        refused(hiplib, f(p, 40, 40, 3, F32, 3, 2000, 20, t, 3500, k, d, nn), "dtype must be MI_U8 or MI_U16")
        refused(hiplib, f(p, 40, 40, 3, U8, 0, 2000, 20, t, 3500, k, d, nn), "levels must be in [1, 8]")
        refused(hiplib, f(p, 40, 40, 3, U8, 9, 2000, 20, t, 3500, k, d, nn), "levels must be in [1, 8]")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 0, 20, t, 3500, k, d, nn), "n_features must be in [1, 65536]")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 65537, 20, t, 3500, k, d, nn), "n_features must be in [1, 65536]")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 2000, 255, t, 3500, k, d, nn), "threshold must be in [0, 254]")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 2000, 20, None, 3500, k, d, nn), "null pattern")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 2000, 20, far.ctypes.data, 3500, k, d, nn), "pattern[32767] must be within 13")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 2000, 20, t, 3499, k, d, nn), "max_kp must hold")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 2000, 20, t, 3500, None, d, nn), "null keypoint array")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 2000, 20, t, 3500, k, None, nn), "null descriptor array")
        refused(hiplib, f(p, 40, 40, 3, U8, 3, 2000, 20, t, 3500, k, d, None), "null n_kp")
    assert n.value == -7                                        # a refused call writes nothing


def test_match_checks(hiplib):
    lib = hiplib.load()
    d = np.zeros((4, 32), np.uint8)
    o = np.zeros((4, 3), np.int32)
    p, q = d.ctypes.data, o.ctypes.data
    for dev in (False, True):
        f = (lambda *x: lib.mi_feat_match_device(0, None, *x)) if dev else (lambda *x: lib.mi_feat_match(0, *x))
        refused(hiplib, f(None, 4, p, 4, q), "null query descriptors")
        refused(hiplib, f(p, 4, None, 4, q), "null train descriptors")
        refused(hiplib, f(p, 0, p, 4, q), "nq must be in")
        refused(hiplib, f(p, (1 << 20) + 1, p, 4, q), "nq must be in")
        refused(hiplib, f(p, 4, p, 0, q), "nt must be in")
        refused(hiplib, f(p, 4, p, (1 << 20) + 1, q), "nt must be in")
        refused(hiplib, f(p, 4, p, 4, None), "null match output")


def test_ransac_checks(hiplib):
    lib = hiplib.load()
    src = np.arange(16, dtype=np.float64).reshape(8, 2) ** 2
    dst = src + 1.0
    sam = np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int32)
    cnt = np.zeros(2, np.int32)
    mod = np.zeros((2, 9))
    s, d, t, c, m = (x.ctypes.data for x in (src, dst, sam, cnt, mod))
    for dev in (False, True):
        f = (lambda *x: lib.mi_feat_ransac_device(0, None, *x)) if dev else (lambda *x: lib.mi_feat_ransac(0, *x))
        refused(hiplib, f(None, d, 8, t, 2, 1, 3.0, c, m), "null source points")
        refused(hiplib, f(s, None, 8, t, 2, 1, 3.0, c, m), "null destination points")
        refused(hiplib, f(s, d, 8, t, 2, 2, 3.0, c, m), "unknown model 2")
        refused(hiplib, f(s, d, 3, t, 2, 1, 3.0, c, m), "n must be in [4,")
        refused(hiplib, f(s, d, 1, t, 2, 0, 3.0, c, m), "n must be in [2,")
        refused(hiplib, f(s, d, (1 << 24) + 1, t, 2, 0, 3.0, c, m), "n must be in [2,")
        refused(hiplib, f(s, d, 8, None, 2, 1, 3.0, c, m), "null sample table")
        refused(hiplib, f(s, d, 8, t, 0, 1, 3.0, c, m), "k must be in")
        refused(hiplib, f(s, d, 8, t, (1 << 20) + 1, 1, 3.0, c, m), "k must be in")
        refused(hiplib, f(s, d, 8, t, 2, 1, 0.0, c, m), "thr must be finite and > 0")
        refused(hiplib, f(s, d, 8, t, 2, 1, float("nan"), c, m), "thr must be finite and > 0")
        refused(hiplib, f(s, d, 8, t, 2, 1, float("inf"), c, m), "thr must be finite and > 0")
        refused(hiplib, f(s, d, 8, t, 2, 1, 3.0, None, m), "null counts")
        refused(hiplib, f(s, d, 8, t, 2, 1, 3.0, c, None), "null models")
    # the host form reads its arrays: a point that is not finite and a sample index out of range are named too
    bad = src.copy()
    bad[5, 1] = np.inf
    refused(hiplib, lib.mi_feat_ransac(0, bad.ctypes.data, d, 8, t, 2, 1, 3.0, c, m), "point 5 must be finite")
    refused(hiplib, lib.mi_feat_ransac(0, s, bad.ctypes.data, 8, t, 2, 1, 3.0, c, m), "point 5 must be finite")
    far = sam.copy()
    far[1, 2] = 8
    refused(hiplib, lib.mi_feat_ransac(0, s, d, 8, far.ctypes.data, 2, 1, 3.0, c, m), "sample 2 of hypothesis 1 must be in [0, 8)")
    far[1, 2] = -1
    refused(hiplib, lib.mi_feat_ransac(0, s, d, 8, far.ctypes.data, 2, 1, 3.0, c, m), "sample 2 of hypothesis 1 must be in [0, 8)")


def test_python_layer_maps_a_refusal_to_value_error(hiplib):
    """_lib.check turns MI_ERR_INVALID into ValueError with the library's text"""
    lib = hiplib.load()
    with pytest.raises(ValueError, match="null frame"):
        hiplib.check(lib.mi_feat_gray(0, None, 8, 8, 3, U8, None))
