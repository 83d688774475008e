"""GPU: calibration on the mosaic upload path of a stack handle (csrc/mosaic_host.hpp).  Frames pushed with
push_mosaic(m, cfa, calibration=c) must fuse exactly as the same frames calibrated on the host by the restatement
(tests/calib_restatement.py) and pushed with push_mosaic as they are: the fused image and the level-0 winner-index tap are
array_equal.  Eight frames -- twice MosaicStage::NSLOT, so every device slot is used again -- with batch_frames = 3: two full
batches and a tail of two.  The calibration itself is held to its restatement by test_gpu_calib.py."""
import numpy as np
import pytest

import calib_cases as K
import calib_restatement as C
from test_gpu_mosaic_stack import make_mosaics

pytestmark = pytest.mark.gpu

N = 8
NSLOT = 4                                   # MosaicStage::NSLOT of csrc/mosaic_host.hpp
MIN_SIZE = 8                                # the pyramid's smallest level: frames 40 rows high still have levels to fuse
CASES = {"small u16": (40, 150, np.uint16, "RGGB"), "small u8": (41, 149, np.uint8, "GBRG"),
         "ragged u16": K.RAGGED + (np.uint16, "GRBG"), "ragged u8": K.RAGGED + (np.uint8, "BGGR")}
CAMERA = [[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [0.05, -0.55, 1.5]]


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


@pytest.fixture(scope="module")
def data(dev):
    """per case: (cfa, calibration, develop, raw mosaics, mosaics calibrated by the restatement)"""
    from shinestacker_amd import Calibration, Cfa, Develop
    d = {}
    for name, (h, w, dtype, pattern) in CASES.items():
        mx = K.maxv(dtype)
        bpp = tuple(K.black_per_position(dtype))
        cfa = Cfa(pattern, black=list(bpp), gains=[1.8, 1.0, 1.0, 1.4])
        dark, flat = K.ordinary_dark((h, w), dtype), K.falloff_flat((h, w), dtype, bpp)
        gain = C.flat_gain(flat, bpp)
        scene = make_mosaics(h, w, dtype, N, seed=h)
        # what the sensor delivers: the scene under the flat's shading, on the dark's fixed pattern
        shade = C.flat_signal(flat, bpp).astype(np.float64)
        shade /= shade.max()
        raw = [np.clip(m * shade * 0.8 + dark, 0, mx).astype(dtype) for m in scene]
        mask = np.random.default_rng(w).random((h, w)) < 0.01
        for m in raw:
            m[mask] = mx
        calibrated = [C.calibrate(m, bpp, dark, gain) for m in raw]
        assert not np.array_equal(calibrated[0], raw[0])
        d[name] = (cfa, Calibration(dark=dark, flat=flat), Develop(matrix=CAMERA, tone="srgb", defects=mask), raw, calibrated)
    yield d
    for v in d.values():
        v[1].close()
        v[2].close()


def run(lib, st, cfa, cal, develop, raw, calibrated, kinds, zero_copy=False):
    """push frame k as: 'c' raw with calibration=, 'C' raw with calibration= and develop=, 'h' host-calibrated plain, 'H'
    host-calibrated with develop=; (fused image, level-0 winner indices)"""
    keep = []
    for k, kind in enumerate(kinds):
        src = (raw if kind in "cC" else calibrated)[k]
        if zero_copy:
            pinned = lib.host_alloc(src.shape, src.dtype)
            pinned[...] = src
            keep.append(pinned)
            src = pinned
        kw = {}
        if kind in "cC":
            kw["calibration"] = cal
        if kind in "CH":
            kw["develop"] = develop
        st.push_mosaic(src, cfa, zero_copy=zero_copy, **kw)
        assert st.frames_pushed == k + 1
    if zero_copy:
        st.wait_uploads(0)
    idx = st.tap(lib.TAP_INDEX, 0)
    return st.finish(), idx


def new_stack(lib, case, **kw):
    h, w, dtype, _ = CASES[case]
    return lib.Stack(h, w, in_dtype=dtype, batch_frames=3, min_size=MIN_SIZE, **kw)


@pytest.mark.parametrize("zero_copy", [False, True], ids=["pageable", "zero_copy"])
@pytest.mark.parametrize("case", list(CASES))
def test_calibrated_mosaics_fuse_as_host_calibrated_ones(dev, data, case, zero_copy):
    args = data[case]
    assert N > NSLOT
    with new_stack(dev, case) as st:
        for plain, with_cal in (("h", "c"), ("H", "C")):                 # without and with develop=
            want, want_idx = run(dev, st, *args, plain * N)
            assert len(np.unique(want_idx)) > 3                          # the winners come from many frames
            st.reset()
            got, got_idx = run(dev, st, *args, with_cal * N, zero_copy=zero_copy)
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want), with_cal
            assert not st._calibrations and not st._develops             # finish let go of both
            st.reset()
        # the calibration matters: the raw mosaics fuse to another image
        raw_args = args[:4] + (args[3],)
        other, _ = run(dev, st, *raw_args, "h" * N)
        assert not np.array_equal(other, want)
    # a handle that only ever saw calibrated mosaics
    with new_stack(dev, case) as st:
        want, want_idx = run(dev, st, *args, "h" * N)
    with new_stack(dev, case) as st:
        got, got_idx = run(dev, st, *args, "c" * N, zero_copy=zero_copy)
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)


@pytest.mark.parametrize("case", list(CASES))
def test_plain_developed_and_calibrated_pushes_mix(dev, data, case):
    """frame by frame on one handle; 'h' and 'H' are plain and developed pushes of today's kind"""
    args = data[case]
    with new_stack(dev, case) as st:
        for kinds, same in (("chCHchCH", "hhHHhhHH"), ("ccHhCCch", "hhHhHHhh"), ("hCcHHcCh", "hHhHHhHh")):
            want, want_idx = run(dev, st, *args, same)
            st.reset()
            got, got_idx = run(dev, st, *args, kinds)
            st.reset()
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want), kinds
        # a plain push after calibrated ones is the plain push again
        st.push_mosaic(args[3][0], args[0], calibration=args[1])
        assert len(st._calibrations) == 1 and st._calibrations[0] is args[1]
        st.reset()
        assert not st._calibrations
        raw_args = args[:4] + (args[3],)
        with new_stack(dev, case) as fresh:
            want, want_idx = run(dev, fresh, *raw_args, "h" * N)
        got, got_idx = run(dev, st, *raw_args, "h" * N)
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)


@pytest.mark.parametrize("case", ["small u16", "ragged u8"])
@pytest.mark.parametrize("how", ["simple", "f64"])
def test_synchronous_routes(dev, data, how, case):
    """MI_IMPL_SIMPLE and float-64 handles: upload, calibration, defects, (developed) demosaic, push, wait"""
    args = data[case][:3] + (data[case][3][:4], data[case][4][:4])
    kw = dict(impl=dev.IMPL_SIMPLE) if how == "simple" else dict(float_type=dev.MI_F64)
    with new_stack(dev, case, **kw) as st:
        for kinds, same in (("cccc", "hhhh"), ("CCCC", "HHHH"), ("cHCh", "hHHh")):
            want, want_idx = run(dev, st, *args, same)
            st.reset()
            got, got_idx = run(dev, st, *args, kinds)
            st.reset()
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want), kinds


def test_push_rejects_misuse(dev, data):
    from shinestacker_amd import Calibration, InvalidOptionError
    from shinestacker_amd.errors import BitDepthError
    cfa, cal, develop, raw, calibrated = data["small u8"]
    with new_stack(dev, "small u8") as st:
        with pytest.raises(InvalidOptionError):
            st.push_mosaic(raw[0], cfa, calibration="dark.tif")
        with pytest.raises(InvalidOptionError):
            st.push_mosaic(raw[0], cfa, calibration=Calibration(dark=np.zeros((8, 8), np.uint8)))
        with pytest.raises(BitDepthError):
            st.push_mosaic(raw[0], cfa, calibration=Calibration(dark=np.zeros(raw[0].shape, np.uint16)))
        assert st.frames_pushed == 0 and not st._calibrations


def test_the_handle_checks_its_arguments(dev, data):
    """mi_stack_push_mosaic_calibrated on a live handle: MI_ERR_INVALID with the argument named, and nothing is pushed"""
    import ctypes
    lib = dev.load()
    cfa, cal, develop, raw, calibrated = data["small u8"]
    c = ctypes.byref(cfa.struct(np.uint8))
    m = np.ascontiguousarray(raw[0])
    good = cal.prepared(m.shape, np.uint8, cfa)

    def calib(flags, dark=good.dev_dark, gain=good.dev_gain):
        return ctypes.byref(dev.CalibStruct(flags, dark, gain))

    with new_stack(dev, "small u8") as st:
        for args, msg in (((st._h, None, 0, c, calib(3), None, None, 0, 0), b"null mosaic"),
                          ((st._h, m.ctypes.data, 0, None, calib(3), None, None, 0, 0), b"null cfa"),
                          ((st._h, m.ctypes.data, 0, c, None, None, None, 0, 0), b"null calib"),
                          ((st._h, m.ctypes.data, 0, c, calib(8), None, None, 0, 0), b"unknown calib flags 8"),
                          ((st._h, m.ctypes.data, 0, c, calib(1, None), None, None, 0, 0), b"MI_CALIB_DARK is set and dev_dark is null"),
                          ((st._h, m.ctypes.data, 0, c, calib(2, gain=None), None, None, 0, 0), b"MI_CALIB_FLAT is set and dev_gain is null"),
                          ((st._h, m.ctypes.data, 0, c, calib(3), None, None, 5, 0), b"null sites"),
                          ((st._h, m.ctypes.data, 0, c, calib(3), None, None, -1, 0), b"number of sites must be >= 0"),
                          ((st._h, m.ctypes.data, m.shape[1] - 1, c, calib(3), None, None, 0, 0), b"row stride smaller than a row"),
                          ((st._h, m.ctypes.data, 0, c, calib(3), ctypes.byref(dev.DevelopStruct(2)), None, 0, 0),
                           b"MI_DEVELOP_TONE is set and dev_tone is null")):
            assert lib.mi_stack_push_mosaic_calibrated(*args) == dev.MI_ERR_INVALID, msg
            assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())
        assert st.frames_pushed == 0
        # no flag set: the plain push
        dev.check(lib.mi_stack_push_mosaic_calibrated(st._h, m.ctypes.data, 0, c, calib(0, None, None), None, None, 0, 0))
        got = st.finish()
        st.reset()
        st.push_mosaic(m, cfa)
        assert np.array_equal(st.finish(), got)


@pytest.mark.parametrize("case", list(CASES))
def test_focus_stack_arrays_calibrates_mosaics(dev, data, case):
    from shinestacker_amd import PyramidStack
    cfa, cal, develop, raw, calibrated = data[case]
    algo = PyramidStack(batch_frames=3, min_size=MIN_SIZE)
    try:
        want = algo.focus_stack_arrays(calibrated, mosaic=cfa)
        got = algo.focus_stack_arrays(raw, mosaic=cfa, calibration=cal)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert not np.array_equal(got, algo.focus_stack_arrays(raw, mosaic=cfa))
        want = algo.focus_stack_arrays(calibrated, mosaic=cfa, develop=develop)
        got = algo.focus_stack_arrays(raw, mosaic=cfa, develop=develop, calibration=cal)
        assert np.array_equal(got, want)
    finally:
        algo.close()


@pytest.mark.parametrize("case", ["small u16", "ragged u8"])
def test_bunches_then_stack_calibrates_mosaics(dev, data, case):
    from shinestacker_amd import pipeline
    cfa, cal, develop, raw, calibrated = data[case]
    h, w, dtype, _ = CASES[case]
    taps = {"h": [], "c": []}
    want, bunches = pipeline.bunches_then_stack(lambda i: calibrated[i], N, h, w, dtype, frames=4, overlap=2, batch_frames=3, min_size=MIN_SIZE, mosaic=cfa,
                                                on_final=lambda st, buf: taps["h"].append(st.tap(dev.TAP_INDEX, 0)))
    got, bunches_c = pipeline.bunches_then_stack(lambda i: raw[i], N, h, w, dtype, frames=4, overlap=2, batch_frames=3, min_size=MIN_SIZE, mosaic=cfa,
                                                 calibration=cal, on_final=lambda st, buf: taps["c"].append(st.tap(dev.TAP_INDEX, 0)))
    assert bunches == bunches_c and len(bunches) > 2
    assert np.array_equal(taps["c"][0], taps["h"][0]) and np.array_equal(got, want)
    got, _ = pipeline.bunches_then_stack(lambda i: raw[i], N, h, w, dtype, frames=4, overlap=2, batch_frames=3, min_size=MIN_SIZE, mosaic=cfa,
                                         calibration=cal, develop=develop)
    want, _ = pipeline.bunches_then_stack(lambda i: calibrated[i], N, h, w, dtype, frames=4, overlap=2, batch_frames=3, min_size=MIN_SIZE, mosaic=cfa,
                                          develop=develop)
    assert np.array_equal(got, want)
