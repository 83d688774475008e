"""CPU: the resident feature estimator's C boundary -- mi_feat_aligner_* declared in include/mi355stack.h, exported by the
library, bound in _lib.SIGNATURES with as many arguments as the header gives them, and every argument check that can be
reached without a device answered with MI_ERR_INVALID and the argument's name before any device call.  create checks all of
its arguments before it looks for a device, so all of them are checked here; the other entry points need a handle, which only
a device gives: here they are refused for a null handle, and tests/test_gpu_feature_aligner.py::test_call_order_and_tap_range
walks their remaining arguments (estimate_batch before set_reference and the tap ranges among them) on a real handle."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["mi_feat_aligner_create", "mi_feat_aligner_set_reference", "mi_feat_aligner_estimate_batch", "mi_feat_aligner_tap",
         "mi_feat_aligner_stats", "mi_feat_aligner_destroy"]
U8, U16, F32 = 0, 1, 2


def _header():
    text = open(os.path.join(ROOT, "include", "mi355stack.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(hiplib, name):
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    m = re.search(rf"MI_API int {name}\((.*?)\);", _header(), flags=re.S)
    assert m, f"{name} is not declared"
    assert hasattr(lib, name), f"{name} is not exported"
    assert name in hiplib.SIGNATURES
    assert len(hiplib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name


def test_enums_match_the_header(hiplib):
    text = _header()
    for i, stage in enumerate(("GRAY", "CUT", "KP", "DESC", "GOOD", "SAMPLES", "COUNTS")):
        assert re.search(rf"MI_FEAT_TAP_{stage} = {i}\b", text) and getattr(hiplib, "FEAT_TAP_" + stage) == i
    assert re.search(r"MI_FEAT_MATCH_KNN = 0, MI_FEAT_MATCH_HAMMING = 1", text)
    assert (hiplib.FEAT_MATCH_KNN, hiplib.FEAT_MATCH_HAMMING) == (0, 1)
    assert hiplib.FeatureAligner.MAX_BATCH == 128 and hiplib.FeatureAligner.MAX_FEATURES == 4096


def refused(hiplib, rc, text):
    assert rc == hiplib.MI_ERR_INVALID
    assert text in hiplib.load().mi_last_error().decode(), hiplib.load().mi_last_error()


def test_create_checks(hiplib):
    from shinestacker_amd import features as ft
    lib = hiplib.load()
    pat = np.array(ft.pattern())
    far = pat.copy()
    far[0, 3, 1] = -14
    t = pat.ctypes.data
    h = ctypes.c_void_p(5)
    out = ctypes.byref(h)

    def f(*a):
        return lib.mi_feat_aligner_create(*a)
    ok = dict(device=0, height=240, width=320, dtype=U8, channels=3, subsample=2, fast=0, levels=3, n_features=2000, threshold=20,
              pattern=t, max_batch=16)

    def call(**kw):
        return f(out, *{**ok, **kw}.values())
    refused(hiplib, f(None, *ok.values()), "null handle pointer")
    refused(hiplib, call(height=0), "height and width must be >= 1")
    refused(hiplib, call(width=-3), "height and width must be >= 1")
    refused(hiplib, call(width=32769), "must be <= 32768")
    refused(hiplib, call(dtype=F32), "dtype must be MI_U8 or MI_U16")
    refused(hiplib, call(channels=2), "channels must be 1 or 3")
    refused(hiplib, call(subsample=0), "subsample must be in [1, 64]")
    refused(hiplib, call(subsample=65), "subsample must be in [1, 64]")
    refused(hiplib, call(subsample=3), "fast must be set for subsample 3")
    refused(hiplib, call(height=241), "fast must be set for subsample 2 on a 320x241 frame")
    refused(hiplib, call(width=321), "fast must be set for subsample 2")
    refused(hiplib, call(levels=0), "levels must be in [1, 8]")
    refused(hiplib, call(levels=9), "levels must be in [1, 8]")
    refused(hiplib, call(n_features=0), "n_features must be in [1, 4096]")
    refused(hiplib, call(n_features=4097), "n_features must be in [1, 4096] on a handle (got 4097)")
    refused(hiplib, call(threshold=255), "threshold must be in [0, 254]")
    refused(hiplib, call(threshold=-1), "threshold must be in [0, 254]")
    refused(hiplib, call(pattern=None), "null pattern")
    refused(hiplib, call(pattern=far.ctypes.data), "pattern[13] must be within 13 (got -14)")
    refused(hiplib, call(max_batch=0), "max_batch must be in [1, 128] (got 0)")
    refused(hiplib, call(max_batch=129), "max_batch must be in [1, 128] (got 129)")
    assert h.value is None                                      # a refused create leaves a null handle behind
    # what is accepted gets as far as looking for a device: no refusal of an argument
    for kw in ({}, {"n_features": 4096}, {"max_batch": 128}, {"max_batch": 1}, {"subsample": 3, "fast": 1},
               {"height": 241, "subsample": 1}, {"channels": 1, "dtype": U16}):
        assert call(**kw) != hiplib.MI_ERR_INVALID, kw
        if h.value:
            lib.mi_feat_aligner_destroy(h)
            h.value = None


def test_a_null_handle_is_refused_everywhere(hiplib):
    lib = hiplib.load()
    buf = np.zeros(64, np.uint8)
    n = ctypes.c_int(-7)
    w, k = ctypes.c_uint64(9), ctypes.c_uint64(9)
    ptrs = (ctypes.c_void_p * 1)(buf.ctypes.data)
    p = buf.ctypes.data
    refused(hiplib, lib.mi_feat_aligner_set_reference(None, p), "null handle")
    refused(hiplib, lib.mi_feat_aligner_estimate_batch(None, ptrs, 1, 0, 0.75, 0, 3.0, 100, 0, 3500, p, p, p, p, p, p, p), "null handle")
    refused(hiplib, lib.mi_feat_aligner_tap(None, 0, 0, 0, p, 64, ctypes.byref(n)), "null handle")
    refused(hiplib, lib.mi_feat_aligner_stats(None, ctypes.byref(w), ctypes.byref(k)), "null handle")
    assert lib.mi_feat_aligner_destroy(None) == hiplib.MI_OK    # as free(NULL)
    assert n.value == -7 and (w.value, k.value) == (9, 9)       # a refused call writes nothing


def test_python_layer_refuses_before_the_library(hiplib):
    from shinestacker_amd import features as ft
    from shinestacker_amd.errors import InvalidOptionError
    with pytest.raises(ValueError, match="n_features must be in"):
        hiplib.FeatureAligner(64, 64, np.uint8, ft.pattern(), n_features=4097)
    with pytest.raises(ValueError, match="max_batch must be in"):
        hiplib.FeatureAligner(64, 64, np.uint8, ft.pattern(), max_batch=129)
    with pytest.raises(ValueError, match="32 x 256 x 4"):
        hiplib.FeatureAligner(64, 64, np.uint8, np.zeros(7, np.int8))
    with pytest.raises(InvalidOptionError, match="4096"):
        ft.FeatureAligner(64, 64, np.uint8, ft.FeatureParams(3, 4097, 20))
    for bad in (0, 129, True, 2.0):
        with pytest.raises(InvalidOptionError, match="max_batch"):
            ft.FeatureAligner(64, 64, np.uint8, max_batch=bad)
