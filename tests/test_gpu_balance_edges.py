"""GPU: the balance kernels (csrc/kernels_balance.hpp: hist_u8 / hist_u16, lut_apply_u8 / _u16, lut_linear_build,
cvt_color_u8) equal the oracle (oracle/oracle.py: balance_hist, resize_area_int, apply_lut, cvt_color_u8) and the
restatement of the table build (balance_cases.linear_table) on the cases of tests/balance_cases.py -- which
test_balance_cases_host.py shows to be meaningful: grids past every launcher's cap, all 256^3 colours through all four
conversions, the histogram's edge grids, partial blocks and points on the mask's circle, every tail and alignment of the
table apply, and the linear table's empty interval, clipping and black frame.  Every comparison is array_equal.

The device forms run between two guard bands of 0xA5 that must come back untouched, as must every buffer the call only
reads."""
import ctypes as C

import numpy as np
import pytest

import balance_cases as B

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of a device buffer; a multiple of 4, so `shift` alone decides the alignment
FILL = 0xA5
DTYPES = pytest.mark.parametrize("dtype", B.DTYPES, ids=B.dtype_name)
MODES = pytest.mark.parametrize("lumi", [False, True], ids=["bgr", "lumi"])


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())


class Band:
    """`nbytes` of device memory `shift` bytes past a 256-byte boundary, between two guard bands; the payload is `arr`, or
    the guard's fill where the call is to write all of it (or nothing)"""

    def __init__(self, dev, arr, nbytes, shift):
        self.arr = None if arr is None else np.ascontiguousarray(arr)
        self.nbytes = self.arr.nbytes if arr is not None else int(nbytes)
        self.at = GUARD + shift
        self.buf = dev.DeviceBuffer(self.at + self.nbytes + GUARD)
        self.buf.upload(np.full(self.buf.nbytes, FILL, np.uint8))
        if self.arr is not None:
            self.buf.upload(self.arr, self.at)
        self.ptr = self.buf.ptr + self.at

    def raw(self):
        """the payload's bytes, after the check that neither guard band was written"""
        raw = self.buf.download((self.buf.nbytes,), np.uint8)
        assert (raw[:self.at] == FILL).all() and (raw[self.at + self.nbytes:] == FILL).all(), "a guard band was written"
        return raw[self.at:self.at + self.nbytes].copy()

    def read(self, shape, dtype):
        return self.raw().view(dtype).reshape(shape)

    def assert_unchanged(self, what):
        assert np.array_equal(self.raw(), self.arr.reshape(-1).view(np.uint8)), f"{what} is only read, and changed"


class Bands:
    """the device buffers of one call, freed together"""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.all:
            b.buf.free()

    def put(self, arr, shift=0):
        self.all.append(Band(self.dev, arr, None, shift))
        return self.all[-1]

    def empty(self, nbytes, shift=0):
        self.all.append(Band(self.dev, None, nbytes, shift))
        return self.all[-1]

    def sync(self):
        self.dev.check(self.dev.load().mi_device_synchronize(0))


def code_of(dev, dtype):
    return dev.DTYPE_CODE[np.dtype(dtype)]


# ---------------------------------------------------------------------------------------------- histograms
def hist_device(dev, img, lumi, s, fast, mask):
    """mi_histogram_device on a scratch of exactly nch * nbins words: the counts it returns are the words it left there"""
    h, w = img.shape[:2]
    nch, nb = (1 if lumi else 3), B.nbins_of(img.dtype)
    counts = np.full((nch, nb), -1, np.int64)
    with Bands(dev) as d:
        src, scr = d.put(img), d.empty(nch * nb * 4)
        dev.check(dev.load().mi_histogram_device(0, None, src.ptr, scr.ptr, h, w, code_of(dev, img.dtype), int(lumi), s, int(fast),
                                                 float(mask), counts.ctypes.data))
        d.sync()
        assert np.array_equal(scr.read((nch, nb), np.uint32), counts), "the scratch and the returned counts differ"
        src.assert_unchanged("the frame")
    return counts


@DTYPES
@MODES
def test_histogram_edge_grids_partial_blocks_masks_and_constant_frames(dev, oracle, dtype, lumi):
    """1 x 1 grids, dropped and kept partial blocks, area means at s = 3, 5, 6, 7, masks with grid points on the circle,
    frames whose every atomic lands on one word: host form and device form"""
    for case in B.HIST_CASES:
        img, want = B.hist_frame(case, dtype), B.hist_reference(oracle, case, dtype, lumi)
        mode = dev.HIST_LUMI if lumi else dev.HIST_BGR
        assert_same((case.name, "host"), dev.histogram(img, mode, case.s, case.fast, case.mask), want)
        assert_same((case.name, "device"), hist_device(dev, img, lumi, case.s, case.fast, case.mask), want)


@DTYPES
def test_histogram_area_mean_past_the_grid_cap(dev, oracle, dtype):
    """725 x 730 sub-sampled pixels > 2048 workgroups x 256: the grid-stride loop of the area-mean path, plain and masked"""
    for case in B.LONG_HIST_CASES:
        img = B.hist_frame(case, dtype)
        for lumi in (False, True):
            want = B.hist_reference(oracle, case, dtype, lumi)
            assert_same((case.name, lumi), hist_device(dev, img, lumi, case.s, case.fast, case.mask), want)


@DTYPES
@MODES
def test_histogram_batch_slices_and_scratch_stride(dev, oracle, dtype, lumi):
    """mi_histogram_device_batch: slice k of the counts and of the scratch is frame k's histogram, at stride nch * nbins,
    and the scratch past the last slice keeps its fill"""
    frames = B.batch_frames(dtype)
    h, w = B.BATCH_SHAPE
    nch, nb, n, spare = (1 if lumi else 3), B.nbins_of(dtype), len(frames), 1024
    per = nch * nb
    for s, fast, mask in ((1, True, 0.0), (2, False, 0.9)):
        counts = np.full((n, nch, nb), -1, np.int64)
        with Bands(dev) as d:
            srcs = [d.put(f) for f in frames]
            scr = d.empty((n * per + spare) * 4)
            ptrs = (C.c_void_p * n)(*[b.ptr for b in srcs])
            dev.check(dev.load().mi_histogram_device_batch(0, None, ptrs, n, scr.ptr, h, w, code_of(dev, dtype), int(lumi), s,
                                                           int(fast), float(mask), counts.ctypes.data))
            d.sync()
            words = scr.read((n * per + spare,), np.uint32)
            for k, b in enumerate(srcs):
                b.assert_unchanged(f"frame {k}")
        assert (words[n * per:] == 0xA5A5A5A5).all(), "the scratch past the used slices was written"
        assert np.array_equal(words[:n * per].reshape(n, nch, nb), counts)
        for k, f in enumerate(frames):
            assert_same((k, s, fast, mask), counts[k], oracle.balance_hist(f, lumi, s, fast, mask))


# ---------------------------------------------------------------------------------------------- table apply
def lut_device(dev, img, luts, in_place, shift=0):
    h, w = img.shape[:2]
    with Bands(dev) as d:
        src, tab = d.put(img, shift), d.put(luts)
        dst = src if in_place else d.empty(img.nbytes, shift)
        dev.check(dev.load().mi_apply_lut_device(0, None, src.ptr, dst.ptr, h * w, code_of(dev, img.dtype), tab.ptr, luts.shape[0]))
        d.sync()
        got = dst.read(img.shape, img.dtype)
        tab.assert_unchanged("the table")
        if not in_place:
            src.assert_unchanged("the source")
    return got


@DTYPES
@pytest.mark.parametrize("nlut", [1, 3])
def test_apply_lut_every_tail_table_and_form(dev, oracle, dtype, nlut):
    """n % 12 in {0, 3, 6, 9} with and without whole steps in front, random / identity / one-value tables; host form, device
    form out of place and in place (how the pipeline calls it); uint16 also 2 bytes off the 4-byte boundary"""
    for shape in B.LUT_SHAPES:
        img = B.random_frame(shape, dtype, seed=31)
        for kind in B.LUT_KINDS:
            luts = B.lut_tables(kind, dtype, nlut)
            want = oracle.apply_lut(img, luts)
            name = (shape, kind)
            assert_same(name + ("host",), dev.apply_lut(img, luts), want)
            assert_same(name + ("device",), lut_device(dev, img, luts, False), want)
            assert_same(name + ("in place",), lut_device(dev, img, luts, True), want)
            if np.dtype(dtype) == np.uint16:
                assert_same(name + ("2 bytes off",), lut_device(dev, img, luts, False, shift=2), want)
                assert_same(name + ("2 bytes off, in place",), lut_device(dev, img, luts, True, shift=2), want)


@DTYPES
def test_apply_lut_past_the_grid_cap(dev, oracle, dtype):
    """more elements than 4096 workgroups cover in one pass (uint8: x 12 bytes per thread): the grid-stride loops, out of place and
    in place"""
    img = B.random_frame(B.LONG_LUT_SHAPE[dtype], dtype, seed=32)
    luts = B.lut_tables("random", dtype, 3)
    want = oracle.apply_lut(img, luts)
    assert_same("device", lut_device(dev, img, luts, False), want)
    assert_same("in place", lut_device(dev, img, luts, True), want)


def test_apply_lut_refuses_uint8_frames_off_the_dword_boundary(dev):
    """source or destination 1, 2 or 3 bytes off: MI_ERR_INVALID with the reason, before any launch -- nothing is written"""
    img = B.random_frame((37, 53), np.uint8, seed=31)
    luts = B.lut_tables("random", np.uint8, 3)
    lib = dev.load()
    for off in (1, 2, 3):
        for src_off, dst_off, in_place in ((off, 0, False), (0, off, False), (off, off, False), (off, off, True)):
            with Bands(dev) as d:
                src, tab = d.put(img, src_off), d.put(luts)
                dst = src if in_place else d.empty(img.nbytes, dst_off)
                rc = lib.mi_apply_lut_device(0, None, src.ptr, dst.ptr, 37 * 53, dev.MI_U8, tab.ptr, 3)
                assert rc == dev.MI_ERR_INVALID and "4-byte aligned" in dev.last_error(), (src_off, dst_off, in_place)
                d.sync()
                src.assert_unchanged("the source")
                if not in_place:
                    assert (dst.raw() == FILL).all(), "a refused call wrote its destination"


# ---------------------------------------------------------------------------------------------- colour conversions
@pytest.mark.parametrize("code", [0, 1, 2, 3], ids=["bgr2hsv", "hsv2bgr", "bgr2hls", "hls2bgr"])
def test_cvt_color_whole_cube(dev, oracle, code):
    """all 256^3 triples in one call of 4096 x 4096 pixels (16 times the grid cap): every colour, and for the inverse codes every
    hue 0..255 -- 180..255 is the colour of hue 0 --, out of place and in place; compared in slabs of 32 values of channel 0"""
    cube = B.cube()
    lib = dev.load()
    with Bands(dev) as d:
        src, dst = d.put(cube), d.empty(cube.nbytes)
        dev.check(lib.mi_cvt_color_device(0, None, src.ptr, dst.ptr, cube.shape[0] * cube.shape[1], dev.MI_U8, code))
        d.sync()
        got = dst.read(cube.shape, np.uint8)
        dev.check(lib.mi_cvt_color_device(0, None, src.ptr, src.ptr, cube.shape[0] * cube.shape[1], dev.MI_U8, code))
        d.sync()
        assert np.array_equal(src.read(cube.shape, np.uint8), got), "in place differs from out of place"
    for y0, y1 in B.cube_slabs():
        want = oracle.cvt_color_u8(cube[y0:y1], code)
        bad = np.argwhere((got[y0:y1] != want).any(axis=-1))
        assert bad.size == 0, (code, len(bad), [(cube[y0 + y, x].tolist(), got[y0 + y, x].tolist(), want[y, x].tolist()) for y, x in bad[:5]])


# ---------------------------------------------------------------------------------------------- linear tables
@DTYPES
@MODES
def test_linear_table_build_and_apply(dev, oracle, dtype, lumi):
    """mi_balance_linear_device stage by stage: the histogram it leaves == oracle.balance_hist, the table == linear_table, the
    factors == its ratios, the frame == oracle.apply_lut through that table.  An interval without counts (identity, ratio 1),
    a table that clips, first_channel = 1, area mean with a mask, and a black frame, whose entry 0 is the product 0 * inf: 0"""
    lib = dev.load()
    h, w = B.LINEAR_SHAPE
    nb, ntab, size = B.nbins_of(dtype), (1 if lumi else 3), np.dtype(dtype).itemsize
    for case in B.linear_cases(dtype, lumi):
        frame, refs, tables, ratios, want = B.linear_expectation(oracle, case, dtype, lumi)
        ref = (C.c_double * 3)(*(refs + [0.0] * (3 - len(refs))))
        with Bands(dev) as d:
            img, scr, lut, corr = d.put(frame), d.empty(ntab * nb * 4), d.empty(ntab * nb * size), d.empty(8 * len(refs))
            dev.check(lib.mi_balance_linear_device(0, None, img.ptr, scr.ptr, lut.ptr, h, w, code_of(dev, dtype), int(lumi), case.s,
                                                   int(case.fast), float(case.mask), case.lo, case.hi, case.first, ref, corr.ptr))
            d.sync()
            got_hist = scr.read((ntab, nb), np.uint32)
            got_tables = lut.read((ntab, nb), dtype)
            got_ratios = corr.read((len(refs),), np.float64)
            got = img.read(frame.shape, dtype)
        assert_same((case.name, "histogram"), got_hist.astype(np.int64), oracle.balance_hist(frame, lumi, case.s, case.fast, case.mask))
        assert_same((case.name, "table"), got_tables, tables)
        assert np.array_equal(got_ratios, ratios, equal_nan=True), (case.name, got_ratios, ratios)
        assert_same((case.name, "frame"), got, want)
        if case.name == "black":
            assert (got_tables[:, 0] == 0).all() and not got.any()
