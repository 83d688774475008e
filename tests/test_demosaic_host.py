"""CPU: the demosaic's NumPy restatement (tests/demosaic_restatement.py) has the properties that make it a demosaic, the cases
the GPU test runs exercise both clamps, Cfa validates and quantises, the tile constants of the kernel and of the Python module
agree, and the C boundary rejects bad arguments before it looks for a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import demosaic_cases as dc
import demosaic_restatement as R
from conftest import ROOT
from shinestacker_amd import Cfa, InvalidOptionError
from shinestacker_amd import demosaic as D

SHAPES = [(2, 2), (2, 7), (3, 3), (5, 2), (17, 33), (64, 65)]
SWAP_RB = {"RGGB": "BGGR", "BGGR": "RGGB", "GRBG": "GBRG", "GBRG": "GRBG"}


def swap_columns(p):
    return p[1] + p[0] + p[3] + p[2]


def swap_rows(p):
    return p[2:] + p[:2]


def random_mosaic(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, size=shape).astype(dtype)


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_restatement_properties(pattern, dtype):
    mx = int(np.iinfo(dtype).max)
    for k, shape in enumerate(SHAPES):
        h, w = shape
        m = random_mosaic(shape, dtype, 100 + k)
        out = R.demosaic(m, pattern)
        assert out.dtype == m.dtype and out.shape == shape + (3,)
        # (a) a mosaic sampled from a constant-colour frame gives that frame back
        for colour in ((0, 0, 0), (mx, mx, mx), (mx, 0, mx // 3), (1, mx - 1, 7)):
            frame = np.broadcast_to(np.array(colour, dtype), shape + (3,))
            assert np.array_equal(R.demosaic(R.mosaic_of(frame, pattern), pattern), frame), (shape, colour)
        # (b) the output sampled at its own sites gives the mosaic back
        assert np.array_equal(R.mosaic_of(out, pattern), m), shape
        # (c) swapping R and B in the pattern swaps the output's channels
        assert np.array_equal(R.demosaic(m, SWAP_RB[pattern]), out[..., ::-1]), shape
        # (d) a frame linear in x and y is reproduced exactly two pixels inside the border
        if h > 4 and w > 4:
            y, x = np.mgrid[0:h, 0:w]
            frame = np.stack([3 + x + 2 * y, 40 + 2 * x + y, 11 + x + y], axis=-1)
            assert frame.max() <= mx
            frame = frame.astype(dtype)
            got = R.demosaic(R.mosaic_of(frame, pattern), pattern)
            assert np.array_equal(got[2:-2, 2:-2], frame[2:-2, 2:-2]), shape
        # (e) dropping the first column (row) and exchanging the pattern's columns (rows) gives the same interior
        if w >= 4:
            assert np.array_equal(R.demosaic(m[:, 1:], swap_columns(pattern))[:, 2:], out[:, 3:]), shape
        if h >= 4:
            assert np.array_equal(R.demosaic(m[1:], swap_rows(pattern))[2:], out[3:]), shape


def test_mosaic_of_matches_the_restatements_and_the_pattern():
    frame = random_mosaic((6, 8, 3), np.uint16, 5)
    for p in R.PATTERNS:
        assert np.array_equal(D.mosaic_of(frame, p), R.mosaic_of(frame, p))
    m = D.mosaic_of(frame, "GRBG")
    assert m[0, 0] == frame[0, 0, 1] and m[0, 1] == frame[0, 1, 2] and m[1, 0] == frame[1, 0, 0] and m[1, 1] == frame[1, 1, 1]
    with pytest.raises(InvalidOptionError):
        D.mosaic_of(frame, "RGBG")
    with pytest.raises(InvalidOptionError):
        D.mosaic_of(frame[..., 0], "RGGB")


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_both_clamps_act_on_the_gpu_tests_random_cases(pattern, dtype):
    """A kernel that forgot a clamp (or shifted logically) must not pass test_gpu_demosaic.py: on every random case of a
    tile or more, sums below 0 and sums above white both occur."""
    mx = int(np.iinfo(dtype).max)
    for shape in dc.BIG_ENOUGH:
        _, sums = dc.reference(shape, dtype, pattern, True)
        r = (sums + 8) >> 4
        assert (r < 0).sum() > 0 and (r > mx).sum() > 0, (shape, int((r < 0).sum()), int((r > mx).sum()))


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_option_cases_move_the_result(dtype):
    """the per-site corrections of the option cases change the output, and step A's clamp acts where white is lowered"""
    for name, m, cfa in dc.option_cases(dtype):
        code, black, gain_q, white = cfa.quantised(dtype)
        want = dc.restate(m, cfa)
        assert want.max() <= white, name
        if m.any() and (any(black) or any(g != D.GAIN_ONE for g in gain_q) or white != np.iinfo(dtype).max):
            assert not np.array_equal(want, R.demosaic(m, R.PATTERNS[code])), name
        if "gains 0" == name or "all zero" == name:
            assert not want.any(), name
        if name == "all maximum":
            assert (want == np.iinfo(dtype).max).all()


def test_cfa_validation_and_quantisation():
    c = Cfa()
    assert c.quantised(np.uint8) == (0, (0, 0, 0, 0), (4096,) * 4, 255)
    assert c.quantised(np.uint16) == (0, (0, 0, 0, 0), (4096,) * 4, 65535)
    assert Cfa(gains=15.99).quantised()[2] == (65495,) * 4
    assert Cfa("gbrg", black=64, gains=2).quantised(np.uint16) == (3, (64,) * 4, (8192,) * 4, 65535)
    assert Cfa("BGGR", black=[1, 2, 3, 4], gains=[0.0, 0.5, 1.0001, 2.5], white=4095).quantised(np.uint16) == \
        (1, (1, 2, 3, 4), (0, 2048, 4096, 10240), 4095)
    assert [Cfa(p).quantised()[0] for p in ("RGGB", "BGGR", "GRBG", "GBRG")] == [0, 1, 2, 3]
    s = Cfa("GRBG", black=[1, 2, 3, 4], gains=[1, 2, 3, 4], white=200).struct(np.uint8)
    assert (s.pattern, list(s.black), list(s.gain_q), s.white) == (2, [1, 2, 3, 4], [4096, 8192, 12288, 16384], 200)
    for bad in (dict(pattern="RGBG"), dict(pattern=0), dict(gains=16.0), dict(gains=15.9999), dict(gains=-0.1), dict(gains=float("nan")),
                dict(gains=[1.0, 1.0, 1.0]), dict(gains="1"), dict(black=-1), dict(black=1.5), dict(black=[0, 0, 0]),
                dict(black=[0, 0, 0, -2]), dict(white=0), dict(white=65536), dict(white=100.0), dict(white=True)):
        with pytest.raises(InvalidOptionError):
            Cfa(**bad)
    with pytest.raises(InvalidOptionError):
        Cfa(white=256).quantised(np.uint8)
    assert Cfa(white=256).quantised(np.uint16)[3] == 256


def test_tile_constants_match_the_kernel_header():
    text = open(os.path.join(ROOT, "shinestacker_amd", "csrc", "kernels_demosaic.hpp")).read()
    th = re.search(r"constexpr int TILE_H = (\d+);", text)
    tw = re.search(r"constexpr int TILE_W = (\d+);", text)
    assert th and tw
    assert (int(th.group(1)), int(tw.group(1))) == (D.TILE_H, D.TILE_W)
    assert D.TILE_H % 2 == 0 and D.TILE_W % 4 == 0      # whole cells per thread: one (uint16) or two side by side (uint8)


def test_c_boundary_is_declared_exported_bound_and_checks_before_any_device_call(hiplib):
    from test_abi import header_symbols
    names = ("mi_demosaic", "mi_demosaic_device", "mi_stack_push_mosaic")
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in names:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name)
    text = open(os.path.join(ROOT, "include", "mi355stack.h")).read()
    for i, p in enumerate(D.PATTERNS):
        assert re.search(rf"MI_CFA_{p} = {i}\b", text)
    lib = hiplib.load()
    assert lib.mi_abi_version() == 1
    m = np.zeros((4, 6), np.uint16)
    out = np.zeros((4, 6, 3), np.uint16)
    U8, U16, F32 = hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32

    def cfa(**kw):
        s = Cfa().struct(np.uint16)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return ctypes.byref(s)

    mp, op = m.ctypes.data, out.ctypes.data
    bad = [((None, op, 4, 6, U16, cfa()), b"null mosaic"),
           ((mp, None, 4, 6, U16, cfa()), b"null bgr"),
           ((mp, op, 4, 6, U16, None), b"null cfa"),
           ((mp, op, 1, 6, U16, cfa()), b"height and width must be >= 2"),
           ((mp, op, 4, 1, U16, cfa()), b"height and width must be >= 2"),
           ((mp, op, 4, 6, F32, cfa()), b"dtype must be MI_U8 or MI_U16"),
           ((mp, op, 4, 6, U16, cfa(pattern=4)), b"unknown cfa pattern 4"),
           ((mp, op, 4, 6, U16, cfa(pattern=-1)), b"unknown cfa pattern -1"),
           ((mp, op, 4, 6, U16, cfa(black=(2, -1))), b"black[2] must be >= 0"),
           ((mp, op, 4, 6, U16, cfa(gain_q=(3, 65536))), b"gain_q[3] must be <= 65535"),
           ((mp, op, 4, 6, U16, cfa(white=0)), b"white must be in [1, 65535]"),
           ((mp, op, 4, 6, U16, cfa(white=65536)), b"white must be in [1, 65535]"),
           ((mp, op, 4, 6, U8, cfa(white=256)), b"white must be in [1, 255]")]
    for args, msg in bad:
        assert lib.mi_demosaic(0, *args) == hiplib.MI_ERR_INVALID, msg
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())
        assert lib.mi_demosaic_device(0, None, *args) == hiplib.MI_ERR_INVALID, msg
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())
    assert lib.mi_stack_push_mosaic(None, mp, 0, cfa(), 0) == hiplib.MI_ERR_INVALID
    assert b"null handle" in lib.mi_last_error()
