"""GPU: the demosaic kernel (csrc/kernels_demosaic.hpp) equals its NumPy restatement (tests/demosaic_restatement.py) bit for bit
on the cases of tests/demosaic_cases.py: the smallest frames, frames that end on a tile edge, one site before it and one past
it, several tiles with a ragged last one -- four patterns x {uint8, uint16} on seeded full-range random mosaics (which put sums
below 0 and above white, test_demosaic_host.py) -- and the per-site corrections at the ragged shape.  Every comparison is
array_equal."""
import numpy as np
import pytest

import demosaic_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def debayer_on_device(lib, mosaic, cfa, offset=0):
    """debayer_device on buffers of the test's own; `offset`: bytes by which the output frame is shifted in its buffer (the
    kernel picks its store path by the row's address); the bytes around the frame must stay as they were"""
    from shinestacker_amd.demosaic import debayer_device
    h, w = mosaic.shape
    nb = mosaic.nbytes * 3
    guard = 64
    src, dst = lib.DeviceBuffer(mosaic.nbytes), lib.DeviceBuffer(nb + 2 * guard)
    try:
        src.upload(mosaic)
        fill = np.full(nb + 2 * guard, 0xA5, np.uint8)
        dst.upload(fill)
        debayer_device(src.ptr, dst.ptr + guard + offset, h, w, mosaic.dtype, cfa)
        lib.check(lib.load().mi_device_synchronize(0))
        raw = dst.download((nb + 2 * guard,), np.uint8)
        assert (raw[:guard + offset] == 0xA5).all() and (raw[guard + offset + nb:] == 0xA5).all(), "wrote outside the frame"
        assert np.array_equal(src.download(mosaic.shape, mosaic.dtype), mosaic)
        return raw[guard + offset:guard + offset + nb].view(mosaic.dtype).reshape(h, w, 3)
    finally:
        src.free()
        dst.free()


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("pattern", dc.PATTERNS)
def test_demosaic_equals_the_restatement(dev, pattern, dtype):
    from shinestacker_amd import Cfa, debayer
    for shape in dc.SHAPES:
        got = debayer(dc.random_mosaic(shape, dtype), Cfa(pattern))
        assert_same((pattern, np.dtype(dtype).name, shape), got, dc.reference(shape, dtype, pattern))


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_black_gains_white_and_saturated_mosaics(dev, dtype):
    from shinestacker_amd import debayer
    for name, m, cfa in dc.option_cases(dtype):
        assert_same((name, np.dtype(dtype).name), debayer(m, cfa), dc.restate(m, cfa))


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_device_form_equals_host_form_at_every_row_alignment(dev, dtype):
    """the device form on the caller's buffers; an output frame that starts 0 .. 3 samples into a 4-byte word takes the
    12-byte stores on other rows (or on none), and nothing outside the frame is written"""
    from shinestacker_amd import Cfa, debayer
    isz = np.dtype(dtype).itemsize
    for shape in ((dc.TH + 1, dc.TW + 1), (dc.TH + 1, dc.TW + 2), dc.RAGGED):
        m = dc.random_mosaic(shape, dtype)
        host = debayer(m, Cfa("GBRG"))
        assert_same(("host", shape), host, dc.reference(shape, dtype, "GBRG"))
        for k in range(4 // isz):
            assert_same(("device", shape, k), debayer_on_device(dev, m, Cfa("GBRG"), offset=k * isz), host)


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_frames_side_by_side_equal_single_calls(dev, dtype):
    from shinestacker_amd import Cfa, debayer
    from shinestacker_amd.demosaic import debayer_frames_device
    cfa = Cfa("BGGR", black=3, gains=[1.5, 1.0, 1.0, 2.0])
    mosaics = [dc.random_mosaic(dc.RAGGED, dtype, salt=10 + i) for i in range(3)]
    want = np.stack([debayer(m, cfa) for m in mosaics])
    for i, m in enumerate(mosaics):
        assert_same(i, want[i], dc.restate(m, cfa))
    buf = dev.DeviceBuffer(want.nbytes)
    try:
        debayer_frames_device(mosaics, buf.ptr, cfa)
        assert_same("side by side", buf.download(want.shape, want.dtype), want)
    finally:
        buf.free()


def test_python_rejects_what_is_no_mosaic(dev):
    from shinestacker_amd import Cfa, InvalidOptionError, debayer
    from shinestacker_amd.errors import BitDepthError
    with pytest.raises(InvalidOptionError):
        debayer(np.zeros((4, 4, 3), np.uint8), Cfa())
    with pytest.raises(InvalidOptionError):
        debayer(np.zeros((1, 4), np.uint8), Cfa())
    with pytest.raises(BitDepthError):
        debayer(np.zeros((4, 4), np.float32), Cfa())
    with pytest.raises(InvalidOptionError):
        debayer(np.zeros((4, 4), np.uint8), "RGGB")
