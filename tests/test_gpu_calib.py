"""GPU: raw calibration (csrc/kernels_calib.hpp: mosaic_master, flat_sums / flat_gain_table, mosaic_calibrate) equals its NumPy
restatement (tests/calib_restatement.py) bit for bit on the cases of tests/calib_cases.py -- which test_calib_host.py shows to
be meaningful -- in host form and in device form, the device forms on the null stream and on a handle's stream.  Every
comparison is array_equal."""
import ctypes

import numpy as np
import pytest

import calib_cases as K
import calib_restatement as C
import develop_restatement as DR
from demosaic_cases import restate as restate_demosaic

pytestmark = pytest.mark.gpu

DTYPES = K.DTYPES
GUARD = 256         # bytes on either side of a device buffer, a multiple of the kernel's 16-byte window


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


@pytest.fixture(scope="module")
def side(dev):
    """a handle whose stream serves as the non-null stream of the device forms"""
    st = dev.Stack(64, 64)
    assert st.stream
    yield st
    st.close()


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def cfa_of(black, pattern="RGGB"):
    from shinestacker_amd import Cfa
    return Cfa(pattern, black=list(black))


def wait(dev, side, stream):
    if stream:
        side.sync()
    else:
        dev.check(dev.load().mi_device_synchronize(0))


def master_device(dev, side, frames, reject, stream=None):
    k, (h, w), dt = len(frames), frames[0].shape, frames[0].dtype
    src, dst = dev.DeviceBuffer(k * frames[0].nbytes), dev.DeviceBuffer(frames[0].nbytes)
    try:
        src.upload(np.stack(frames))
        dev.check(dev.load().mi_mosaic_master_device(0, stream, src.ptr, k, h, w, dev.DTYPE_CODE[dt], reject, dst.ptr))
        wait(dev, side, stream)
        return dst.download((h, w), dt)
    finally:
        src.free()
        dst.free()


def flat_gain_device(dev, side, flat, black, fdark, stream=None):
    h, w = flat.shape
    c = cfa_of(black).struct(flat.dtype)
    src, dst = dev.DeviceBuffer(flat.nbytes), dev.DeviceBuffer(h * w * 2)
    fd = None if fdark is None else dev.DeviceBuffer(fdark.nbytes)
    try:
        src.upload(flat)
        if fd is not None:
            fd.upload(fdark)
        dev.check(dev.load().mi_flat_gain_device(0, stream, src.ptr, None if fd is None else fd.ptr, h, w, dev.DTYPE_CODE[flat.dtype],
                                                 ctypes.byref(c), dst.ptr))
        wait(dev, side, stream)
        return dst.download((h, w), np.uint16)
    finally:
        for b in (src, dst, fd):
            if b is not None:
                b.free()


def calibrate_device(dev, side, mosaic, black, dark, gain, stream=None, shift=0):
    """in place on a mosaic that starts `shift` sites off the 16-byte boundary, between two guard bands; the tables likewise"""
    h, w = mosaic.shape
    c = cfa_of(black).struct(mosaic.dtype)
    bufs, at = {}, {}
    try:
        for name, a in (("m", mosaic), ("d", dark), ("g", gain)):
            if a is not None:
                at[name] = GUARD + shift * a.itemsize
                b = bufs[name] = dev.DeviceBuffer(a.nbytes + 2 * GUARD + shift * a.itemsize)
                b.upload(np.full(b.nbytes, 0xA5, np.uint8))
                b.upload(a, at[name])
        cal = dev.CalibStruct((dev.MI_CALIB_DARK if dark is not None else 0) | (dev.MI_CALIB_FLAT if gain is not None else 0),
                              bufs["d"].ptr + at["d"] if dark is not None else None,
                              bufs["g"].ptr + at["g"] if gain is not None else None)
        dev.check(dev.load().mi_mosaic_calibrate_device(0, stream, bufs["m"].ptr + at["m"], h, w, dev.DTYPE_CODE[mosaic.dtype],
                                                        ctypes.byref(c), ctypes.byref(cal)))
        wait(dev, side, stream)
        raw = bufs["m"].download((bufs["m"].nbytes,), np.uint8)
        lo, hi = at["m"], at["m"] + mosaic.nbytes
        assert (raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all(), "the guard band around the mosaic was written"
        for name, a in (("d", dark), ("g", gain)):      # the tables are only read
            if a is not None:
                assert np.array_equal(bufs[name].download((a.nbytes,), np.uint8, at[name]), np.ascontiguousarray(a).reshape(-1).view(np.uint8)), name
        return raw[lo:hi].copy().view(mosaic.dtype).reshape(h, w)
    finally:
        for b in bufs.values():
            b.free()


# ---------------------------------------------------------------------------------------------- master frames
@pytest.mark.parametrize("dtype", DTYPES)
def test_master_every_k_and_reject(dev, side, dtype):
    """every (K, reject) at the ragged shape (20723 sites: the per-sample path) and at a multiple of 4 sites (the vector path)"""
    from shinestacker_amd import master_frame
    for shape in (K.RAGGED, (16, 24), K.SMALL_ODD):
        for k, r in K.MASTER_CASES:
            frames = K.random_frames(shape, dtype, k)
            want = K.master_reference(shape, dtype, k, r)
            name = (np.dtype(dtype).name, shape, k, r)
            assert_same(name + ("host",), master_frame(list(frames), reject=r), want)
            assert_same(name + ("device",), master_device(dev, side, frames, r), want)
    k, r = 9, 2
    assert_same("stream", master_device(dev, side, K.random_frames(K.RAGGED, dtype, k), r, side.stream), K.master_reference(K.RAGGED, dtype, k, r))
    assert_same("stream", master_device(dev, side, K.random_frames((16, 24), dtype, k), r, side.stream), K.master_reference((16, 24), dtype, k, r))


@pytest.mark.parametrize("dtype", DTYPES)
def test_master_every_shape(dev, side, dtype):
    from shinestacker_amd import master_frame
    for i, shape in enumerate(K.shapes(dtype)):
        for k, r in ((5, 1), (9, 4), (17, 0)):
            frames = K.random_frames(shape, dtype, k)
            want = K.master_reference(shape, dtype, k, r)
            assert_same((shape, k, r, "host"), master_frame(np.stack(frames), reject={4: "median", 0: "mean"}.get(r, r)), want)
            assert_same((shape, k, r, "device"), master_device(dev, side, frames, r, side.stream if i & 1 else None), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_master_outliers_identical_and_saturated_sets(dev, side, dtype):
    from shinestacker_amd import master_frame
    for name, frames, r in K.special_master_sets(dtype):
        want = C.master(frames, r)
        assert_same((name, "host"), master_frame(list(frames), reject=r), want)
        assert_same((name, "device"), master_device(dev, side, frames, r), want)


# ---------------------------------------------------------------------------------------------- flat gain tables
@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_gain_every_case(dev, side, dtype):
    from shinestacker_amd import flat_gain
    for name, flat, black, fdark in K.flat_cases(dtype):
        want = C.flat_gain(flat, black, fdark)
        assert_same((name, "host"), flat_gain(flat, cfa_of(black), fdark), want)
        assert_same((name, "device"), flat_gain_device(dev, side, flat, black, fdark), want)
        assert_same((name, "stream"), flat_gain_device(dev, side, flat, black, fdark, side.stream), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_gain_every_shape(dev, side, dtype):
    from shinestacker_amd import flat_gain
    bpp = tuple(K.black_per_position(dtype))
    for i, shape in enumerate(K.shapes(dtype)):
        flat = K.falloff_flat(shape, dtype, bpp)
        want = K.falloff_gain(shape, dtype, bpp)
        assert_same((shape, "host"), flat_gain(flat, cfa_of(bpp, "GBRG")), want)
        assert_same((shape, "device"), flat_gain_device(dev, side, flat, bpp, None, side.stream if i & 1 else None), want)
        fdark = K.ordinary_dark(shape, dtype)
        assert_same((shape, "flat-dark"), flat_gain_device(dev, side, flat, bpp, fdark, None if i & 1 else side.stream),
                    C.flat_gain(flat, bpp, fdark))


# ---------------------------------------------------------------------------------------------- calibrate
def host_calibrate(dev, mosaic, black, dark, gain):
    """mi_mosaic_calibrate with the tables as they are (the Python wrapper builds its gain table from a flat)"""
    out = np.empty_like(mosaic)
    c = cfa_of(black).struct(mosaic.dtype)
    m = np.ascontiguousarray(mosaic)
    dev.check(dev.load().mi_mosaic_calibrate(0, m.ctypes.data, out.ctypes.data, m.shape[0], m.shape[1], dev.DTYPE_CODE[m.dtype],
                                             ctypes.byref(c), None if dark is None else np.ascontiguousarray(dark).ctypes.data,
                                             None if gain is None else np.ascontiguousarray(gain).ctypes.data))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_calibrate_every_shape(dev, side, dtype):
    """dark, flat and both at every shape: host form, device form on both streams, and rows pushed off the 16-byte boundary"""
    for i, shape in enumerate(K.shapes(dtype)):
        for name, m, black, dark, gain in K.shape_cases(shape, dtype):
            want = K.restate(m, black, dark, gain)
            assert_same((shape, name, "host"), host_calibrate(dev, m, black, dark, gain), want)
            assert_same((shape, name, "device"), calibrate_device(dev, side, m, black, dark, gain, side.stream if i & 1 else None), want)
            assert_same((shape, name, "shifted"), calibrate_device(dev, side, m, black, dark, gain, None, shift=1 + i % 5), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_calibrate_every_option_case(dev, side, dtype):
    for name, m, black, dark, gain in K.option_cases(dtype):
        want = K.restate(m, black, dark, gain)
        assert_same((name, "host"), host_calibrate(dev, m, black, dark, gain), want)
        assert_same((name, "device"), calibrate_device(dev, side, m, black, dark, gain), want)
        assert_same((name, "stream"), calibrate_device(dev, side, m, black, dark, gain, side.stream), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_calibration_object(dev, dtype):
    """Calibration reduces its exposures, builds its table against the Cfa and calibrates: each step as the restatement"""
    from shinestacker_amd import Calibration, calibrate
    bpp = tuple(K.black_per_position(dtype))
    cfa = cfa_of(bpp, "GRBG")
    shape = K.RAGGED
    darks = [np.minimum(K.ordinary_dark(shape, dtype), f) for f in K.random_frames(shape, dtype, 5)]
    flats, quiet, _ = K.outlier_frames(shape, dtype)
    fdark = K.ordinary_dark(shape, dtype) // 4
    m = K.random_mosaic(shape, dtype, salt=3)
    for reject, r_d, r_f in (("median", 2, 4), ("mean", 0, 0), (1, 1, 1)):
        d, f = C.master(darks, r_d), C.master(flats, r_f)
        with Calibration(dark=darks, flat=np.stack(flats), flat_dark=fdark, reject=reject) as cal:
            assert_same("master dark", cal.master("dark"), d)
            assert_same("master flat", cal.master("flat"), f)
            g = C.flat_gain(f, bpp, fdark)
            assert_same("gain", cal.gain_table(cfa), g)
            assert_same("calibrate", calibrate(m, cfa, cal), C.calibrate(m, bpp, d, g))
            assert_same("another cfa", calibrate(m, cfa_of((0, 0, 0, 0)), cal), C.calibrate(m, (0, 0, 0, 0), d, C.flat_gain(f, (0, 0, 0, 0), fdark)))
    with Calibration(dark=darks[0]) as cal:
        assert_same("dark only", calibrate(m, cfa, cal), C.calibrate(m, bpp, darks[0], None))
    with Calibration(flat=flats[0]) as cal:
        assert_same("flat only", calibrate(m, cfa, cal), C.calibrate(m, bpp, None, C.flat_gain(flats[0], bpp)))
    with Calibration() as cal:
        assert_same("neither", calibrate(m, cfa, cal), m)


# ---------------------------------------------------------------------------------------------- the order of the steps
@pytest.mark.parametrize("dtype", DTYPES)
def test_debayer_calibrates_first_then_repairs_then_demosaics(dev, dtype):
    from shinestacker_amd import Calibration, Cfa, Develop, debayer
    from develop_cases import MATRICES, tone_table
    mx = K.maxv(dtype)
    for shape in (K.RAGGED, (5, 2 * 16 // np.dtype(dtype).itemsize + 1), (3, 3)):
        bpp = tuple(K.black_per_position(dtype))
        cfa = Cfa("GBRG", black=list(bpp), gains=[1.7, 1.0, 1.0, 1.3])
        m = K.random_mosaic(shape, dtype, salt=3)
        dark, flat = K.ordinary_dark(shape, dtype), K.falloff_flat(shape, dtype, bpp)
        gain = K.falloff_gain(shape, dtype, bpp)
        mask = np.random.default_rng(shape[1]).random(shape) < 0.05
        hot = m.copy()
        hot[mask] = mx
        with Calibration(dark=dark, flat=flat) as cal:
            calibrated = C.calibrate(hot, bpp, dark, gain)
            assert_same((shape, "plain"), debayer(hot, cfa, calibration=cal), restate_demosaic(calibrated, cfa))
            with_dev = Develop(matrix=MATRICES["camera"], tone=tone_table("random", dtype), defects=mask)
            sites = with_dev.sites(shape)
            repaired = DR.defects(calibrated, sites)
            code, black, gain_q, white = cfa.quantised(dtype)
            want = DR.develop(calibrated, "GBRG", black, gain_q, white, DR.quantise_matrix(MATRICES["camera"]), tone_table("random", dtype), sites)
            got = debayer(hot, cfa, develop=with_dev, calibration=cal)
            assert_same((shape, "developed"), got, want)
            if shape == K.RAGGED:
                # the order shows: repairing the raw samples first and calibrating afterwards gives another image
                other = DR.develop(C.calibrate(DR.defects(hot, sites), bpp, dark, gain), "GBRG", black, gain_q, white,
                                   DR.quantise_matrix(MATRICES["camera"]), tone_table("random", dtype), None)
                assert not np.array_equal(other, want) and not np.array_equal(repaired, calibrated)
            with_dev.close()
            # debayer_frames_device: the same, frame by frame into one buffer
            from shinestacker_amd.demosaic import debayer_frames_device
            out = dev.DeviceBuffer(2 * hot.nbytes * 3)
            try:
                debayer_frames_device([hot, m], out.ptr, cfa, calibration=cal)
                both = out.download((2,) + shape + (3,), dtype)
                assert_same((shape, "frames 0"), both[0], restate_demosaic(calibrated, cfa))
                assert_same((shape, "frames 1"), both[1], restate_demosaic(C.calibrate(m, bpp, dark, gain), cfa))
            finally:
                out.free()
