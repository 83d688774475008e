"""GPU: raw development (csrc/kernels_demosaic.hpp: mosaic_defects and the matrix / tone epilogue of demosaic_mhc) equals its NumPy
restatement (tests/develop_restatement.py) bit for bit on the cases of tests/develop_cases.py -- which test_develop_host.py shows
to be meaningful.  Every comparison is array_equal."""
import numpy as np
import pytest

import develop_cases as vc

pytestmark = pytest.mark.gpu

# which steps ride on the demosaic: (matrix?, tone?)
WHICH = {"matrix": (True, False), "tone": (False, True), "both": (True, True)}
MATRIX_NAMES = [n for n in vc.MATRICES]
TONE_NAMES = list(vc.TONES[:5])          # ("white below the maximum" needs its Cfa: test_every_matrix_and_tone_case)


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def make_develop(dtype, matrix=None, tone=None, defects=None):
    from shinestacker_amd import Develop
    return Develop(matrix=None if matrix is None else vc.MATRICES[matrix], tone=None if tone is None else vc.tone_arg(tone, dtype),
                   defects=defects)


@pytest.mark.parametrize("dtype", vc.DTYPES)
@pytest.mark.parametrize("pattern", vc.PATTERNS)
@pytest.mark.parametrize("which", list(WHICH))
def test_developed_demosaic_equals_the_restatement(dev, which, pattern, dtype):
    """every shape; the matrix and the tone table walk through their cases from shape to shape"""
    from shinestacker_amd import Cfa, debayer
    with_m, with_t = WHICH[which]
    for k, shape in enumerate(vc.SHAPES):
        mat = MATRIX_NAMES[(k + 1) % len(MATRIX_NAMES)] if with_m else None
        tone = TONE_NAMES[(k + 1) % len(TONE_NAMES)] if with_t else None
        d = make_develop(dtype, mat, tone)
        got = debayer(vc.random_mosaic(shape, dtype), Cfa(pattern), d)
        assert_same((which, pattern, np.dtype(dtype).name, shape, mat, tone), got, vc.shape_reference(shape, dtype, pattern, mat, tone))


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_every_matrix_and_tone_case(dev, dtype):
    from shinestacker_amd import Cfa, debayer
    m = vc.random_mosaic(vc.RAGGED, dtype)
    for mat in vc.MATRICES:
        assert_same(mat, debayer(m, Cfa("GRBG"), make_develop(dtype, mat)), vc.shape_reference(vc.RAGGED, dtype, "GRBG", mat, None))
    for tone in vc.TONES:
        cfa = vc.tone_cfa(tone, dtype)
        assert_same(tone, debayer(m, cfa, make_develop(dtype, None, tone)), vc.restate(m, cfa, None, vc.tone_table(tone, dtype)))
        assert_same(("camera", tone), debayer(m, cfa, make_develop(dtype, "camera", tone)),
                    vc.restate(m, cfa, vc.MATRICES["camera"], vc.tone_table(tone, dtype)))
    # the identity matrix and the identity table are the plain demosaic
    assert_same("identity", debayer(m, Cfa("GRBG"), make_develop(dtype, "identity", "identity")), debayer(m, Cfa("GRBG")))


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_black_gains_white_and_saturated_mosaics_developed(dev, dtype):
    from shinestacker_amd import debayer
    for which, (with_m, with_t) in WHICH.items():
        mat, tone = "camera" if with_m else None, "random" if with_t else None
        d = make_develop(dtype, mat, tone)
        for name, m, cfa in vc.dc.option_cases(dtype):
            want = vc.restate(m, cfa, None if mat is None else vc.MATRICES[mat], None if tone is None else vc.tone_table(tone, dtype))
            assert_same((name, which, np.dtype(dtype).name), debayer(m, cfa, d), want)


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_defect_kernel_alone(dev, dtype):
    """step 0 in place on a device mosaic: equals the restatement, and no unlisted site is touched"""
    from shinestacker_amd import Develop
    from shinestacker_amd.demosaic import defects_device
    for i, (name, mosaic, sites) in enumerate(vc.defect_cases(dtype)):
        want, ks, lin = vc.defects_reference(dtype, i)
        h, w = mosaic.shape
        guard = 64
        buf = dev.DeviceBuffer(mosaic.nbytes + 2 * guard)
        d = Develop(defects=sites)
        try:
            buf.upload(np.full(mosaic.nbytes + 2 * guard, 0xA5, np.uint8))
            buf.upload(mosaic, guard)
            defects_device(buf.ptr + guard, h, w, dtype, d)
            dev.check(dev.load().mi_device_synchronize(0))
            raw = buf.download((mosaic.nbytes + 2 * guard,), np.uint8)
        finally:
            buf.free()
            d.close()
        assert (raw[:guard] == 0xA5).all() and (raw[guard + mosaic.nbytes:] == 0xA5).all(), name
        got = raw[guard:guard + mosaic.nbytes].view(mosaic.dtype).reshape(h, w)
        assert_same(name, got, want)
        keep = np.ones(h * w, dtype=bool)
        keep[lin] = False
        assert np.array_equal(got.reshape(-1)[keep], mosaic.reshape(-1)[keep]), name


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_defects_through_the_host_form(dev, dtype):
    """debayer(m, cfa, Develop(defects=)) is the plain demosaic of the repaired mosaic, on every defect case"""
    from shinestacker_amd import Cfa, Develop, debayer
    for i, (name, mosaic, sites) in enumerate(vc.defect_cases(dtype)):
        repaired, _, _ = vc.defects_reference(dtype, i)
        cfa = Cfa(vc.PATTERNS[i % 4])
        assert_same(name, debayer(mosaic, cfa, Develop(defects=sites)), vc.dc.restate(repaired, cfa))


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_full_development(dev, dtype):
    """steps 0 to D together"""
    from shinestacker_amd import debayer
    for name, m, cfa, mat, tone, defects in vc.full_cases(dtype):
        got = debayer(m, cfa, make_develop(dtype, mat, tone, defects))
        want = vc.restate(m, cfa, None if mat is None else vc.MATRICES[mat], None if tone is None else vc.tone_table(tone, dtype), defects)
        assert_same((name, np.dtype(dtype).name), got, want)


def develop_on_device(lib, mosaic, cfa, d, offset=0):
    """debayer_device(develop=) on buffers of the test's own, as test_gpu_demosaic.py's debayer_on_device: `offset` shifts the
    output frame in its buffer, the bytes around it must stay as they were.  Returns (bgr, the source mosaic afterwards)."""
    from shinestacker_amd.demosaic import debayer_device
    h, w = mosaic.shape
    nb = mosaic.nbytes * 3
    guard = 64
    src, dst = lib.DeviceBuffer(mosaic.nbytes + 2 * guard), lib.DeviceBuffer(nb + 2 * guard)
    try:
        src.upload(np.full(mosaic.nbytes + 2 * guard, 0x5A, np.uint8))
        src.upload(mosaic, guard)
        dst.upload(np.full(nb + 2 * guard, 0xA5, np.uint8))
        debayer_device(src.ptr + guard, dst.ptr + guard + offset, h, w, mosaic.dtype, cfa, develop=d)
        lib.check(lib.load().mi_device_synchronize(0))
        raw = dst.download((nb + 2 * guard,), np.uint8)
        assert (raw[:guard + offset] == 0xA5).all() and (raw[guard + offset + nb:] == 0xA5).all(), "wrote outside the frame"
        sraw = src.download((mosaic.nbytes + 2 * guard,), np.uint8)
        assert (sraw[:guard] == 0x5A).all() and (sraw[guard + mosaic.nbytes:] == 0x5A).all(), "wrote outside the mosaic"
        return (raw[guard + offset:guard + offset + nb].view(mosaic.dtype).reshape(h, w, 3),
                sraw[guard:guard + mosaic.nbytes].view(mosaic.dtype).reshape(h, w))
    finally:
        src.free()
        dst.free()


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_device_form_equals_host_form_at_every_row_alignment(dev, dtype):
    from shinestacker_amd import Cfa, debayer
    isz = np.dtype(dtype).itemsize
    cfa = Cfa("GBRG")
    for shape in ((vc.TH + 1, vc.TW + 1), (vc.TH + 1, vc.TW + 2), vc.RAGGED):
        m = vc.random_mosaic(shape, dtype)
        mask = np.random.default_rng(shape[1]).random(shape) < 0.02
        lin = vc.linear_sites(mask, shape)
        plain = make_develop(dtype, "camera", "random")
        fixed = make_develop(dtype, "camera", "random", mask)
        try:
            host = debayer(m, cfa, plain)
            assert_same(("host", shape), host, vc.shape_reference(shape, dtype, "GBRG", "camera", "random"))
            host_fixed = debayer(m, cfa, fixed)
            assert_same(("host, defects", shape), host_fixed, vc.restate(m, cfa, vc.MATRICES["camera"], vc.tone_table("random", dtype), mask))
            repaired = vc.DR.defects(m, lin)
            for k in range(4 // isz):
                got, after = develop_on_device(dev, m, cfa, plain, offset=k * isz)
                assert_same(("device", shape, k), got, host)
                assert np.array_equal(after, m), "no defects given: the source mosaic is only read"
                got, after = develop_on_device(dev, m, cfa, fixed, offset=k * isz)
                assert_same(("device, defects", shape, k), got, host_fixed)
                assert_same(("the source, repaired in place", shape, k), after, repaired)
                changed = np.flatnonzero(after.reshape(-1) != m.reshape(-1))
                assert len(changed) and np.isin(changed, lin).all(), "only listed sites are written"
        finally:
            plain.close()
            fixed.close()


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_frames_side_by_side_equal_single_calls(dev, dtype):
    from shinestacker_amd import Cfa, debayer
    from shinestacker_amd.demosaic import debayer_frames_device
    cfa = Cfa("BGGR", black=3, gains=[1.5, 1.0, 1.0, 2.0])
    mask = np.random.default_rng(5).random(vc.RAGGED) < 0.02
    d = make_develop(dtype, "camera", "srgb", mask)
    mosaics = [vc.random_mosaic(vc.RAGGED, dtype, salt=10 + i) for i in range(3)]
    want = np.stack([debayer(m, cfa, d) for m in mosaics])
    assert_same(0, want[0], vc.restate(mosaics[0], cfa, vc.MATRICES["camera"], vc.tone_table("srgb", dtype), mask))
    buf = dev.DeviceBuffer(want.nbytes)
    try:
        debayer_frames_device(mosaics, buf.ptr, cfa, develop=d)
        assert_same("side by side", buf.download(want.shape, want.dtype), want)
    finally:
        buf.free()
        d.close()


def test_python_rejects_misuse(dev):
    from shinestacker_amd import Cfa, Develop, InvalidOptionError, debayer
    from shinestacker_amd.errors import BitDepthError
    m = np.zeros((4, 4), np.uint8)
    with pytest.raises(InvalidOptionError):
        debayer(m, Cfa(), "srgb")
    with pytest.raises(BitDepthError):
        debayer(m, Cfa(), Develop(tone=np.arange(65536).astype(np.uint16)))
    with pytest.raises(InvalidOptionError):
        debayer(m, Cfa(), Develop(defects=[(4, 0)]))
    with pytest.raises(InvalidOptionError):
        debayer(m, Cfa(), Develop(defects=np.zeros((4, 5), bool)))
