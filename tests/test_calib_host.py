"""CPU: the calibration cases of calib_cases.py mean something -- every named case reaches the branch it is named after, checked
with the restatement -- and the Python API validates its options before it asks for a device."""
import numpy as np
import pytest

import calib_cases as K
import calib_restatement as C
from shinestacker_amd import Calibration, Cfa, InvalidOptionError, calibrate, debayer, demosaic, flat_gain, master_frame
from shinestacker_amd.errors import BitDepthError

DTYPES = K.DTYPES


def test_the_shapes_cover_the_kernels_paths():
    for dt in DTYPES:
        v = demosaic.calib_vec(dt)
        th, tw = demosaic.calib_tile(dt)
        assert v * np.dtype(dt).itemsize == demosaic.CALIB_VEC_BYTES == 16 and tw == 64 * v and th == 4
        sh = K.shapes(dt)
        assert len(sh) == len(set(sh)) and all(h >= 2 and w >= 2 for h, w in sh)
        for must in ((2, 2), (3, 3), (4, v - 1), (5, v), (4, v + 1), (5, 2 * v + 1), (th - 1, tw - 1), (th, tw), (th + 1, tw + 1), K.RAGGED):
            assert must in sh, must
        # rows off the 16-byte boundary, and site counts that are no multiple of 4 (the master kernel's per-sample path)
        assert any((w * np.dtype(dt).itemsize) % 16 and h > 1 for h, w in sh) and any((h * w) % 4 for h, w in sh)
        assert any((h * w) % 4 == 0 for h, w in sh)


def test_master_cases_cover_every_k_and_reject():
    assert sorted({k for k, _ in K.MASTER_CASES}) == list(K.KS) == [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32]
    for k in K.KS:
        rs = K.rejects(k)
        assert 0 in rs and (k - 1) // 2 in rs and all(2 * r < k for r in rs)
        assert (1 in rs) == (k > 2)
        if (k - 1) // 2 >= 3:
            assert any(1 < r < (k - 1) // 2 for r in rs)
    # the three definitions agree with the plain statements
    fr = K.random_frames((5, 9), np.uint16, 5)
    st = np.stack(fr).astype(np.int64)
    assert np.array_equal(C.master(fr, 0), (st.sum(0) + 2) // 5)
    assert np.array_equal(C.master(fr, 2), np.median(st, axis=0).astype(np.int64))
    ev = K.random_frames((5, 9), np.uint16, 4)
    s4 = np.sort(np.stack(ev).astype(np.int64), axis=0)
    assert np.array_equal(C.master(ev, 1), (s4[1] + s4[2] + 1) // 2)
    assert np.array_equal(C.master(fr[:1], 0), fr[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_outlier_set_tells_the_rejects_apart(dtype):
    frames, quiet, masks = K.outlier_frames(K.RAGGED, dtype)
    k = len(frames)
    mean, trimmed, median = C.master(frames, 0), C.master(frames, 2), C.master(frames, (k - 1) // 2)
    assert (trimmed != mean).any() and (trimmed != median).any()
    hit = masks[0] | masks[1]
    assert hit.any() and (masks[0] & masks[1]).any() and not hit.all()
    # the hits pull the mean up and are gone from the trimmed result: it stays inside the quiet frames' range
    q = np.stack(quiet).astype(np.int64)
    assert (mean[hit].astype(np.int64) > q.max(0)[hit]).all()
    assert (trimmed >= q.min(0)).all() and (trimmed <= q.max(0)).all()
    # ... and where a site was hit in both frames, rejecting two at each end leaves the outlier-free samples without their two
    # smallest: the mean of those five
    both = masks[0] & masks[1]
    s = np.sort(q[[i for i in range(k) if i not in (2, 5)]], axis=0)      # the seven quiet samples of such a site
    want = (s[2:].sum(0) + 2) // 5
    assert np.array_equal(trimmed[both], want[both])
    # sets without spread: every reject gives the frame itself
    for name, fr, r in K.special_master_sets(dtype):
        if not name.startswith("outliers"):
            assert np.array_equal(C.master(fr, r), fr[0]), name
    assert (C.master(K.saturated_frames(K.RAGGED, dtype), 7) == K.maxv(dtype)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_cases_reach_their_branches(dtype):
    """"Reaches 16384" below means the rule `f == 0 or S_p == 0`, not a site whose value happens to equal its position's mean:
    the plain flats have f > 0 at every site and S_p > 0 at every position, and no gain of theirs clamps."""
    seen = set()
    for name, flat, black, fdark in K.flat_cases(dtype):
        g, sums, counts = C.flat_gain(flat, black, fdark, return_sums=True)
        f = C.flat_signal(flat, black, fdark)
        assert g.dtype == np.uint16 and sum(counts) == flat.size
        if name.startswith("plain"):
            assert f.min() > 0 and min(sums) > 0 and g.max() < 65535, name
            gain = g / 16384.0
            assert 0.70 < gain.min() < 0.80 and 2.4 < gain.max() < 3.2, (name, gain.min(), gain.max())
        if "at and below" in name:
            assert (f == 0).any() and (g[f == 0] == 16384).all() and (f > 0).any() and min(sums) > 0, name
            seen.add("f0")
        if name.startswith(("all black", "all zero")):
            assert sums == [0, 0, 0, 0] and (g == 16384).all(), name
            seen.add("s0")
        if "clamp" in name:
            assert (g == 65535).any() and (g < 65535).any(), name
            seen.add("clamp")
            if fdark is not None:
                assert (f == 0).any() and (g[f == 0] == 16384).all(), name
    assert seen == {"f0", "s0", "clamp"}
    # per-position counts at odd sizes, and the smallest mosaic
    _, _, counts = C.flat_gain(K.falloff_flat(K.RAGGED, dtype), return_sums=True)
    assert counts == [27 * 196, 27 * 195, 26 * 196, 26 * 195]
    _, _, counts = C.flat_gain(np.full((2, 2), 9, dtype), return_sums=True)
    assert counts == [1, 1, 1, 1]
    # the flat-dark replaces the black level altogether
    name, flat, black, fdark = K.flat_cases(dtype)[2]
    assert np.array_equal(C.flat_gain(flat, black, fdark), C.flat_gain(flat, (0, 0, 0, 0), fdark))
    assert not np.array_equal(C.flat_gain(flat, black, fdark), C.flat_gain(flat, black))


@pytest.mark.parametrize("dtype", DTYPES)
def test_calibrate_cases_reach_their_branches(dtype):
    mx = K.maxv(dtype)
    cases = {name: rest for name, *rest in K.option_cases(dtype)}
    # the ordinary case: a dark below maxv / 8 and a fall-off flat leave at least 80 % of the sites unclamped
    m, black, dark, gain = cases["ordinary: dark and flat, black 0"]
    out, e, pre = C.calibrate(m, black, dark, gain, return_parts=True)
    assert dark.max() < mx // 8 + 1
    clamped_hi, clamped_lo = (pre > mx).mean(), (m.astype(np.int64) < dark).mean()
    assert 0.02 < clamped_hi < 0.15 and 0.02 < clamped_lo < 0.10 and clamped_hi + clamped_lo < 0.20, (clamped_hi, clamped_lo)
    # e = 0: a black, or a dark, above the sample
    for name in ("black above some samples, flat", "dark above the sample", "dark above the sample, flat"):
        m, black, dark, gain = cases[name]
        out, e, pre = C.calibrate(m, black, dark, gain, return_parts=True)
        below = m.astype(np.int64) < (C.black_map(m.shape, black) if dark is None else dark.astype(np.int64))
        assert 0.1 < below.mean() < 0.9 and (e[below] == 0).all() and (out[below] == np.minimum(mx, C.black_map(m.shape, black))[below]).all(), name
    # the maxv clamp
    for name in ("gain past maxv", "gain past maxv, dark", "all maxv, dark 0, gain 65535"):
        m, black, dark, gain = cases[name]
        out, e, pre = C.calibrate(m, black, dark, gain, return_parts=True)
        assert (pre > mx).mean() > 0.3 and (out[pre > mx] == mx).all(), name
    m, black, dark, gain = cases["all maxv, dark 0, gain 65535"]
    if dtype == np.uint16:      # the largest product there is: above 2^31, below 2^32 with the rounding term
        assert 2 ** 31 < int((m.astype(np.int64) * gain).max()) + 8192 < 2 ** 32
    # neither table: the mosaic itself
    m, black, dark, gain = cases["neither"]
    assert dark is None and gain is None and np.array_equal(C.calibrate(m, black), m)
    m, black, dark, gain = cases["all zero"]
    assert np.array_equal(C.calibrate(m, black, dark, gain), np.minimum(mx, C.black_map(m.shape, black)))
    # dark, flat and both differ from each other
    a, b, c = (C.calibrate(*cases[n]) for n in ("black per position, dark", "black per position, flat", "black per position, both"))
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pedestal", [False, True], ids=["black 0", "black per position"])
def test_a_flat_calibrated_by_its_own_table_is_constant_per_position(dtype, pedestal):
    """The constant is the position's mean signal S_p / N_p on its pedestal, and every site lies within 2 counts of it: the Q14
    gain is off by at most half a step, e * 0.5 / 16384 <= 1.5 counts at this flat's brightest signal (e < 0.75 * maxv), and the
    calibration's own rounding adds half a count."""
    black = tuple(K.black_per_position(dtype)) if pedestal else (0, 0, 0, 0)
    flat = K.falloff_flat(K.RAGGED, dtype, black)
    gain, sums, counts = C.flat_gain(flat, black, return_sums=True)
    assert np.array_equal(gain, K.falloff_gain(K.RAGGED, dtype, black))
    out = C.calibrate(flat, black, None, gain).astype(np.int64)
    pos = C.position_map(flat.shape)
    assert C.flat_signal(flat, black).max() < 0.75 * K.maxv(dtype)
    for p in range(4):
        v = out[pos == p]
        target = black[p] + sums[p] / counts[p]
        assert np.abs(v - target).max() <= 2, (p, target, v.min(), v.max())
        assert flat[pos == p].max() - flat[pos == p].min() > 20          # (the flat itself is far from constant)


# ---------------------------------------------------------------------------------------------- the API
def frames(k, shape=(6, 8), dtype=np.uint16):
    return [np.full(shape, i, dtype) for i in range(k)]


def test_master_frame_validates_its_options():
    with pytest.raises(BitDepthError):
        master_frame([np.zeros((6, 8), np.float32)] * 3)
    with pytest.raises(BitDepthError):
        master_frame([np.zeros((6, 8), np.uint16), np.zeros((6, 8), np.uint8)])
    with pytest.raises(InvalidOptionError):
        master_frame([np.zeros((6, 8), np.uint16), np.zeros((6, 9), np.uint16)])
    with pytest.raises(InvalidOptionError):
        master_frame([np.zeros((6, 8, 3), np.uint16)])
    with pytest.raises(InvalidOptionError):
        master_frame([])
    with pytest.raises(InvalidOptionError):
        master_frame(frames(33))
    for k, r in ((1, 1), (2, 1), (4, 2), (5, 3), (32, 16), (3, -1)):
        with pytest.raises(InvalidOptionError):
            master_frame(frames(k), reject=r)
    for bad in ("mode", 1.5, None, True):
        with pytest.raises(InvalidOptionError):
            master_frame(frames(5), reject=bad)
    assert demosaic._resolve_reject("mean", 9) == 0 and demosaic._resolve_reject("median", 9) == 4
    assert demosaic._resolve_reject("median", 8) == 3 and demosaic._resolve_reject(3, 8) == 3 and demosaic._resolve_reject("median", 1) == 0


def test_flat_gain_validates_its_options():
    flat = np.full((6, 8), 100, np.uint16)
    with pytest.raises(InvalidOptionError):
        flat_gain(flat, "RGGB")
    with pytest.raises(BitDepthError):
        flat_gain(flat.astype(np.float64), Cfa())
    with pytest.raises(InvalidOptionError):
        flat_gain(flat[:1], Cfa())
    with pytest.raises(InvalidOptionError):
        flat_gain(flat, Cfa(), flat_dark=np.zeros((6, 9), np.uint16))
    with pytest.raises(BitDepthError):
        flat_gain(flat, Cfa(), flat_dark=np.zeros((6, 8), np.uint8))


def test_calibration_validates_its_options():
    d16 = np.zeros((6, 8), np.uint16)
    with pytest.raises(BitDepthError):
        Calibration(dark=d16.astype(np.float32))
    with pytest.raises(BitDepthError):
        Calibration(dark=d16, flat=np.ones((6, 8), np.uint8))
    with pytest.raises(InvalidOptionError):
        Calibration(dark=d16, flat=np.ones((6, 9), np.uint16))
    with pytest.raises(InvalidOptionError):
        Calibration(dark=[d16, np.zeros((6, 9), np.uint16)])
    with pytest.raises(InvalidOptionError):
        Calibration(dark=[])
    with pytest.raises(InvalidOptionError):
        Calibration(flat=frames(33))
    with pytest.raises(InvalidOptionError):
        Calibration(flat=frames(4), reject=2)
    with pytest.raises(InvalidOptionError):
        Calibration(dark=frames(9), flat=frames(2), reject=1)
    with pytest.raises(InvalidOptionError):
        Calibration(dark=d16, reject="mode")
    with pytest.raises(InvalidOptionError):
        Calibration(dark=d16, reject=-1)
    with pytest.raises(InvalidOptionError):
        Calibration(flat_dark=d16)
    c = Calibration(dark=frames(5), flat=np.stack(frames(3)), flat_dark=d16, reject=1)
    assert c.shape == (6, 8) and c.dtype == np.uint16 and "5 frames" in repr(c) and "3 frames" in repr(c) and "master" in repr(c)
    with Calibration() as none:
        assert none.shape is None
    # a calibration of another shape or dtype than the frame: before any device is asked for
    with pytest.raises(InvalidOptionError):
        calibrate(np.zeros((6, 9), np.uint16), Cfa(), c)
    with pytest.raises(BitDepthError):
        calibrate(np.zeros((6, 8), np.uint8), Cfa(), c)
    with pytest.raises(InvalidOptionError):
        c.prepared((8, 6), np.uint16, Cfa())
    with pytest.raises(InvalidOptionError):
        debayer(np.zeros((6, 9), np.uint16), Cfa(), calibration=Calibration(flat=np.ones((6, 8), np.uint16)))
    with pytest.raises(InvalidOptionError):
        calibrate(np.zeros((6, 8), np.uint16), Cfa(), "dark.tif")
    with pytest.raises(InvalidOptionError):
        calibrate(np.zeros((6, 8), np.uint16), "RGGB", c)


def test_calibration_needs_a_mosaic():
    from shinestacker_amd import PyramidStack, pipeline
    c = Calibration(dark=np.zeros((6, 8), np.uint8))
    bgr = [np.zeros((6, 8, 3), np.uint8)] * 2
    with pytest.raises(InvalidOptionError, match="calibration= needs mosaic="):
        PyramidStack().focus_stack_arrays(bgr, calibration=c)
    with pytest.raises(InvalidOptionError, match="calibration= needs mosaic="):
        pipeline.bunches_then_stack(lambda i: bgr[i], 2, 6, 8, np.uint8, calibration=c)
    with pytest.raises(InvalidOptionError):
        PyramidStack().focus_stack_arrays([np.zeros((6, 8), np.uint8)] * 2, mosaic=Cfa(), calibration="dark.tif")
    with pytest.raises(InvalidOptionError):
        demosaic.require_mosaic(None, None, c)
    demosaic.require_mosaic(Cfa(), None, c)
    demosaic.require_mosaic(None, None, None)
