"""GPU: the five kernels of csrc/kernels_prestack.hpp against tests/prestack_restatement.py at the shapes where they branch --
tails, frames narrower than a span, a second trip round a grid-stride loop, every clip of the gain, 1000 hot pixels, windows
larger than the frame, frames smaller than a blur halo, whole tiles -- and the argument checks of their C entry points.
tests/test_prestack_restatement.py pins the restatement to the reference's recordings; test_gpu_prestack.py replays those
recordings through the kernels.

vignette_apply, the undecided-value rule: device exp and NumPy exp need not agree to the last bit.  A value is DECIDED when the
restatement gives the same integer with the unclipped ratio model / v0 scaled by (1 - 2^-44), 1 and (1 + 2^-44); every decided
value must equal the kernel's, an undecided one may differ from the unscaled result by one count.  2^-44 is 16 times the about
2^-48 that two exp calls of at most 1 ulp (the inner result scaled by at most 10 before the outer call) and the divisions can
move the ratio by.  At most 1e-6 of a case's values may be undecided: that is a condition on the case's parameters, asserted
on the restatement before the kernel's output is looked at."""
import ctypes as C

import numpy as np
import pytest

import prestack_restatement as pr
from test_denoise_host import hash_noise

pytestmark = pytest.mark.gpu

REL = 2.0**-44
UNDECIDED_CAP = 1e-6


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


def vmax_of(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else 65535


def make_frame(h, w, dtype, seed, full_range=False, amp=12):
    """integer hash noise over a smooth texture; `full_range` sprinkles 0, 1 and the type's largest value over it"""
    y, x = np.ogrid[:h, :w]
    tex = 120 + 70 * np.sin(x / 17.0 + seed) * np.cos(y / 23.0)
    img = np.rint(tex[:, :, None] * np.array([0.8, 1.0, 0.9])).astype(np.int64) + hash_noise((h, w, 3), seed, amp)
    img = np.clip(img, 0, 255)
    if np.dtype(dtype) == np.uint16:
        img = img * 256 + hash_noise((h, w, 3), seed + 1, 127) + 127
    if full_range:
        sel = hash_noise((h, w, 3), seed + 2, 20)
        img[sel == 20] = vmax_of(dtype)
        img[sel == -20] = 0
        img[sel == 19] = 1
    return img.astype(dtype)


def sync(lib):
    lib.check(lib.load().mi_device_synchronize(0))


# ---------------------------------------------------------------- vignette_apply
def natural(h, w, max_correction=1.0, black_threshold=1.0):
    """parameters of the size a fit gives: the curve falls off at three quarters of the way to the corner"""
    r_max = np.sqrt((w / 2)**2 + (h / 2)**2)
    i0, k, r0 = 360.0, 6.0 / r_max, 0.75 * r_max
    return i0, k, r0, float(pr.model(0.0, i0, k, r0)), max_correction, black_threshold


def expect_vignette(name, img, p, rows=None, height=None):
    """(restatement at rel 0, mask of undecided values); the cap on the undecided share is asserted here"""
    lo, want, hi = (pr.vignette(img, *p, rel=r, rows=rows, height=height) for r in (-REL, 0.0, REL))
    und = (lo != want) | (hi != want)
    share = float(und.mean())
    print(f"vignette {name}: {int(und.sum())} of {und.size} values undecided (share {share:.2e})")
    assert share <= UNDECIDED_CAP, (name, "the case's parameters leave too many values undecided")
    return want, und


def compare_vignette(name, got, want, und):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = (got != want) & ~und
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    assert np.abs(got[und].astype(np.int64) - want[und].astype(np.int64)).max(initial=0) <= 1, name


def apply_vignette(lib, img, p, in_place):
    """the kernel's output, and the source buffer as it is afterwards"""
    from shinestacker_amd import vignetting as vg
    i0, k, r0, v0, mc, bt = p
    src = lib.DeviceBuffer(img.nbytes)
    dst = src if in_place else lib.DeviceBuffer(img.nbytes)
    try:
        src.upload(img)
        if not in_place:
            dst.upload(~img)           # whatever the kernel does not write stays wrong
        vg.vignette_apply_device(src.ptr, dst.ptr, img.shape[0], img.shape[1], img.dtype, (i0, k, r0), v0, mc, bt)
        sync(lib)
        return dst.download(img.shape, img.dtype), src.download(img.shape, img.dtype)
    finally:
        src.free()
        if not in_place:
            dst.free()


def check_vignette(lib, name, img, p):
    want, und = expect_vignette(name, img, p)
    for in_place in (True, False):
        got, src_after = apply_vignette(lib, img, p, in_place)
        compare_vignette((name, in_place), got, want, und)
        if not in_place:
            assert np.array_equal(src_after, img), (name, "the source moved")
    return want


@pytest.mark.parametrize("h,w,dtype", [(203, 301, np.uint16), (37, 53, np.uint8), (5, 7, np.uint8), (5, 7, np.uint16),
                                       (1, 1, np.uint8), (1, 1, np.uint16), (3, 16, np.uint8), (3, 16, np.uint16)])
def test_vignette_tail_and_narrow_frames(dev, h, w, dtype):
    """203 x 301 u16: 7 pixels after the last span; 37 x 53 u8: 9; 5 x 7: fewer pixels than one block's spans, rows wrap inside
    a span; 1 x 1: tail only; 3 x 16 u8: one span per row (u16: two)."""
    pix = 16 if dtype == np.uint8 else 8
    assert (h, w, dtype) != (203, 301, np.uint16) or (h * w) % pix == 7
    assert (h, w, dtype) != (37, 53, np.uint8) or (h * w) % pix == 9
    img = make_frame(h, w, dtype, 3 + h, full_range=h > 1)
    if h == 1:
        img[:] = (200, 90, 150) if dtype == np.uint8 else (51234, 23000, 40001)
    for mc, bt in ((1.0, 1.0), (0.6, 20.0)):
        want = check_vignette(dev, f"{h}x{w} {np.dtype(dtype).name} mc {mc} bt {bt}", img, natural(h, w, mc, bt))
        assert (want != img).any()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_vignette_every_clip_of_the_gain(dev, dtype):
    """240 x 320, k = 0.2, r0 = 100: k (r - r0) runs from -20 to 20, so both clips at +-10 and the cut of exp(t) at 10 are
    reached.  With v0 = model(0) the smallest ratio the clipped model can give is 2 / (1 + e^10) = 9e-5; v0 = 111.8 model(0) (v0
    is a free argument of the entry point; 100 sqrt(1.25), not a power of two, which would put every value of the flat centre on
    an integer and leave it undecided) takes it under 1e-6, the last clip, where every non-zero value saturates.  Then
    k < 0: the ratio is >= 1 everywhere, the gain is clipped to 1 and the output is the input."""
    h, w, BIG = 240, 320, 100 * np.sqrt(1.25)
    img = make_frame(h, w, dtype, 11, full_range=True)
    i0, k, r0 = 360.0, 0.2, 100.0
    y, x = np.ogrid[:h, :w]
    r = np.sqrt((x - w / 2)**2 + (y - h / 2)**2)
    t = k * (r - r0)
    assert t.min() < -10 and t.max() > 10 and np.exp(np.clip(t, -10, 10)).max() > 10
    for scale in (1.0, BIG):
        v0 = scale * float(pr.model(0.0, i0, k, r0))
        ratio = pr.model(r, i0, k, r0) / v0
        assert (ratio.min() < 1e-6) == (scale == BIG)
        want = check_vignette(dev, f"clips {np.dtype(dtype).name} v0 x {scale}", img, (i0, k, r0, v0, 1.0, 0.0))
        if scale == BIG:
            floor = ratio < 1e-6
            assert floor.any() and np.array_equal(want[floor], np.where(img[floor] > 0, vmax_of(dtype), 0))
            assert (want[~floor] < vmax_of(dtype)).any()
    # k < 0
    k = -0.02
    v0 = float(pr.model(0.0, i0, k, r0))
    assert (pr.model(r, i0, k, r0) / v0 >= 1.0).all() and r.min() == 0.0
    want = check_vignette(dev, f"k < 0 {np.dtype(dtype).name}", img, (i0, k, r0, v0, 1.0, 1.0))
    assert np.array_equal(want, img)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_vignette_max_correction_and_black_threshold(dev, dtype):
    """max_correction 1 (no blend), 0.6 and 0 (gain 1 everywhere) x black_threshold 0, 1, 20, on a frame that holds pixels whose
    smallest channel is exactly the threshold (corrected) and one under it (left alone), x 256 for 16-bit."""
    h, w = 240, 320
    scale = 1 if dtype == np.uint8 else 256
    for bt in (0.0, 1.0, 20.0):
        img = make_frame(h, w, dtype, 17, full_range=True)
        t = int(bt) * scale
        for j in range(3):      # the smallest channel in every position
            at = np.roll(np.array([t, t + 7 * scale, t + 30 * scale]), j)
            img[10 + 2 * j, 20:40] = at
            if t >= 1:
                under = at.copy()
                under[j] = t - 1
                img[11 + 2 * j, 20:40] = under
        for mc in (1.0, 0.6, 0.0):
            want = check_vignette(dev, f"{np.dtype(dtype).name} mc {mc} bt {bt}", img, natural(h, w, mc, bt))
            black = img.min(axis=2) < t
            assert black.any() == (bt > 0) and np.array_equal(want[black], img[black])
            if mc == 0.0:
                assert np.array_equal(want, img)
                continue
            for j in range(3):
                assert (want[10 + 2 * j, 20:40] != img[10 + 2 * j, 20:40]).any()
                assert t < 1 or np.array_equal(want[11 + 2 * j, 20:40], img[11 + 2 * j, 20:40])


@pytest.mark.parametrize("h,w,dtype", [(2900, 2900, np.uint16), (3000, 5700, np.uint8)])
def test_vignette_second_trip_round_the_grid(dev, h, w, dtype):
    """The grid is capped at 4096 x 256 threads: these are the smallest frames here with more than 1 048 576 spans, so the last
    threads' loop goes round again.  Compared: the first 64 rows, the last 64 and the 64 rows around the pixel where the second
    trip starts -- into a second buffer (source untouched), then in place."""
    from shinestacker_amd import vignetting as vg
    pix = 16 if dtype == np.uint8 else 8
    first_again = 4096 * 256 * pix
    assert (h * w) // pix > 4096 * 256 and h * w > first_again
    idx = np.arange(h * w * 3, dtype=np.uint32)
    idx ^= idx >> np.uint32(15)
    idx *= np.uint32(0x2c1b3c6d)
    idx ^= idx >> np.uint32(12)
    img = (idx >> np.uint32(8)).astype(dtype).reshape(h, w, 3)
    del idx
    i0, k, r0, v0, mc, bt = p = natural(h, w)
    ya = first_again // w
    blocks = [(0, 64), (max(0, ya - 32), min(h, ya + 32)), (h - 64, h)]
    expected = [expect_vignette(f"{h}x{w} rows {a}-{b}", img[a:b], p, rows=(a, b), height=h) for a, b in blocks]
    row = w * 3 * img.itemsize
    src, dst = dev.DeviceBuffer(img.nbytes), dev.DeviceBuffer(img.nbytes)
    try:
        src.upload(img)
        for a, b in blocks:
            dst.upload(~img[a:b], a * row)
        vg.vignette_apply_device(src.ptr, dst.ptr, h, w, dtype, (i0, k, r0), v0, mc, bt)
        sync(dev)
        for (a, b), (want, und) in zip(blocks, expected):
            compare_vignette((h, w, a, b, "second buffer"), dst.download((b - a, w, 3), dtype, a * row), want, und)
            assert np.array_equal(src.download((b - a, w, 3), dtype, a * row), img[a:b])
            assert (want != img[a:b]).any()
        vg.vignette_apply_device(src.ptr, src.ptr, h, w, dtype, (i0, k, r0), v0, mc, bt)
        sync(dev)
        for (a, b), (want, und) in zip(blocks, expected):
            compare_vignette((h, w, a, b, "in place"), src.download((b - a, w, 3), dtype, a * row), want, und)
    finally:
        src.free()
        dst.free()


# ---------------------------------------------------------------- mask_noise
def hot_layout(h, w, n):
    """a mask of exactly n hot pixels: the four corners, a run along every edge, 3 x 3 clusters (one in a corner), the centres
    of the value regions of mask_noise_frame, and hash-chosen pixels for the rest"""
    mask = np.zeros((h, w), bool)
    mask[0, 0] = mask[0, w - 1] = mask[h - 1, 0] = mask[h - 1, w - 1] = True
    mask[0, 5:40] = mask[h - 1, 60:100] = True
    mask[30:70, 0] = mask[10:50, w - 1] = True
    mask[10:13, 10:13] = mask[50:53, 60:63] = mask[h - 3:, w - 3:] = True
    for y, x in ((25, 25), (45, 25), (61, 21), (61, 41), (75, 25)):
        mask[y, x] = True
    order = np.argsort(hash_noise((h * w,), 5, 1 << 20), kind="stable")
    flat = mask.reshape(-1)
    for i in order:
        if flat.sum() >= n:
            break
        flat[i] = True
    assert mask.sum() == n
    return mask


def mask_noise_frame(dtype):
    """96 x 128 with the value edges: an all-zero region, a region whose only non-zero pixel is the hot one, 3 x 3 windows of 1
    and the largest value (nine values, and eight), a region of one repeated value, and a corner whose four values have two
    middle values an odd amount apart"""
    top = vmax_of(dtype)
    img = make_frame(96, 128, dtype, 23, full_range=True)
    img[20:31, 20:31] = 0
    img[40:51, 20:31] = 0
    img[45, 25] = (7, top, 1)
    pattern = np.where((np.arange(9).reshape(3, 3) % 2 == 0)[:, :, None], 1, top)
    img[60:63, 20:23] = pattern
    img[60:63, 40:43] = pattern
    img[60, 40] = 0
    img[70:81, 20:31] = 77 if dtype == np.uint8 else 77 * 256 + 3
    s = 1 if dtype == np.uint8 else 256
    img[0:2, 0:2] = np.array([[10 * s, 14 * s + (s > 1)], [200 * s, 11 * s]])[:, :, None]
    return img


def run_mask_noise(lib, img, mask, ks, method):
    """(in place through run_frame, into a second buffer through run_frame_device, the source afterwards)"""
    from shinestacker_amd import MaskNoise
    mn = MaskNoise(kernel_size=ks, method=method)
    mn.set_mask(mask.astype(np.uint8))
    src, dst = lib.DeviceBuffer(img.nbytes), lib.DeviceBuffer(img.nbytes)
    try:
        in_place = mn.run_frame(0, 0, img)
        src.upload(img)
        dst.upload(~img)
        mn.run_frame_device(0, src.ptr, img.shape[0], img.shape[1], img.dtype, dev_dst=dst.ptr)
        sync(lib)
        return in_place, dst.download(img.shape, img.dtype), src.download(img.shape, img.dtype)
    finally:
        src.free()
        dst.free()
        mn.end()


@pytest.fixture(scope="module")
def thousand():
    return hot_layout(96, 128, 1000)


@pytest.mark.parametrize("ks", [1, 3, 7, 11])
@pytest.mark.parametrize("method", [pr.MEAN, pr.MEDIAN])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_mask_noise_thousand_hot_pixels(dev, thousand, dtype, method, ks):
    """MAX_NOISY_PIXELS hot pixels (12 workgroups), kernel sizes 1 to 11, every value edge of mask_noise_frame"""
    from shinestacker_amd.noise_detection import MAX_NOISY_PIXELS
    assert thousand.sum() == MAX_NOISY_PIXELS == 1000
    img = mask_noise_frame(dtype)
    coords = np.argwhere(thousand)
    want = pr.mask_noise(img, coords, ks, method)
    # what the frame was built to hold, seen in the restatement
    top = vmax_of(dtype)
    assert not want[25, 25].any() and np.array_equal(want[45, 25], (7, top, 1))
    assert np.array_equal(want[75, 25], img[75, 25]) and len(set(img[75, 25])) == 1
    if ks == 3:
        s = 1 if dtype == np.uint8 else 256
        corner = {pr.MEAN: (235 * s + (s > 1)) // 4, pr.MEDIAN: (25 * s + (s > 1)) // 2}[method]
        assert (want[0, 0] == corner).all() and (method == pr.MEAN or (25 * s + (s > 1)) % 2 == 1)
        assert (want[61, 21] == {pr.MEAN: (5 + 4 * top) // 9, pr.MEDIAN: 1}[method]).all()
        assert (want[61, 41] == (1 + top) // 2).all()
    if ks > 1:
        assert (want[11, 11] != img[11, 11]).any()
    else:
        assert np.array_equal(want, img)
    in_place, second, src_after = run_mask_noise(dev, img, thousand, ks, method)
    assert in_place.dtype == img.dtype and np.array_equal(in_place, want)
    assert np.array_equal(second, want)
    assert np.array_equal(src_after, img)


@pytest.mark.parametrize("method", [pr.MEAN, pr.MEDIAN])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_mask_noise_window_larger_than_the_frame(dev, dtype, method):
    """kernel 31 on 9 x 13: every window is the whole frame"""
    img = make_frame(9, 13, dtype, 29, full_range=True)
    mask = np.zeros((9, 13), bool)
    mask[0, 0] = mask[0, 12] = mask[8, 0] = mask[8, 12] = mask[4, 6] = mask[4, 7] = mask[2, 3] = mask[7, 11] = True
    want = pr.mask_noise(img, np.argwhere(mask), 31, method)
    assert all((want[mask][:, c] == want[0, 0, c]).all() for c in range(3)) and (want != img).any()
    in_place, second, src_after = run_mask_noise(dev, img, mask, 31, method)
    assert np.array_equal(in_place, want) and np.array_equal(second, want) and np.array_equal(src_after, img)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_mask_noise_without_hot_pixels(dev, dtype):
    img = make_frame(37, 53, dtype, 31, full_range=True)
    in_place, second, src_after = run_mask_noise(dev, img, np.zeros((37, 53), bool), 3, pr.MEAN)
    assert np.array_equal(in_place, img) and np.array_equal(second, img) and np.array_equal(src_after, img)


@pytest.mark.parametrize("method", [pr.MEAN, pr.MEDIAN])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_mask_noise_ignores_coordinates_outside_the_frame(dev, dtype, method):
    """mi_mask_noise_device itself: pairs outside the frame (negative, y == h, x == w, far out) change nothing, the pairs
    inside are corrected, no other pixel moves"""
    h, w = 20, 30
    img = make_frame(h, w, dtype, 37, full_range=True)
    coords = np.array([(-1, 5), (3, 4), (h, 3), (4, w), (0, 0), (3, -2), (h - 1, w - 1), (1 << 30, 2), (7, -(1 << 30)), (3, 5),
                       (-h, -w), (12, 17)], np.int32)
    inside = np.array([(3, 4), (0, 0), (h - 1, w - 1), (3, 5), (12, 17)])
    want = pr.mask_noise(img, inside, 3, method)
    assert (want != img).any()
    n = len(coords)
    lib = dev.load()
    src, dst, aux = dev.DeviceBuffer(img.nbytes), dev.DeviceBuffer(img.nbytes), dev.DeviceBuffer(n * 8 + n * 12)
    try:
        src.upload(img)
        dst.upload(~img)
        aux.upload(coords)
        code = dev.DTYPE_CODE[np.dtype(dtype)]
        dev.check(lib.mi_mask_noise_device(0, None, src.ptr, dst.ptr, h, w, code, aux.ptr, n, 3, int(method == pr.MEDIAN), aux.ptr + 8 * n))
        sync(dev)
        assert np.array_equal(dst.download(img.shape, dtype), want)
        assert np.array_equal(src.download(img.shape, dtype), img)
        dev.check(lib.mi_mask_noise_device(0, None, src.ptr, src.ptr, h, w, code, aux.ptr, n, 3, int(method == pr.MEDIAN), aux.ptr + 8 * n))
        sync(dev)
        assert np.array_equal(src.download(img.shape, dtype), want)
    finally:
        for b in (src, dst, aux):
            b.free()


# ---------------------------------------------------------------- frame_accumulate + hot_pixel_map
CHUNKS = {1: [1], 8: [8], 9: [8, 1], 17: [3, 8, 6]}      # frames per _device_add call (at most BATCH)


def noise_frames(h, w, n):
    """n uint8 frames of one scene with their own noise and a few pixels that are hot in one channel or in all; the second
    frame is all 255"""
    frames = []
    for f in range(n):
        fr = make_frame(h, w, np.uint8, 41, amp=0).astype(np.int64) + hash_noise((h, w, 3), 50 + f, 20)
        flat = fr.reshape(-1, 3)
        for j, i in enumerate(range(0, h * w, 53)):
            if j % 4 == 0:
                flat[i] = 250
            else:
                flat[i, j % 3] += 40 + 9 * (j % 7)
        frames.append(np.clip(fr, 0, 255).astype(np.uint8))
    if n > 1:
        frames[1] = np.full((h, w, 3), 255, np.uint8)
    return frames


def thresholds_on_the_data(sums, n, blur_size):
    """per channel a threshold that some pixel's difference EQUALS (the middle one of the values that occur), so that > and >=
    give different maps"""
    mean = (sums.astype(np.int64) // n).astype(np.uint8)
    diff = np.abs(mean.astype(np.int64) - pr.blur(mean, blur_size))
    th = []
    for c in range(3):
        vals = np.unique(diff[..., c])
        th.append(int(vals[len(vals) // 2] if len(vals) > 1 else vals[0]))
        assert (diff[..., c] == th[c]).any()
    return th, diff


def run_noise_detection(frames, chunks, blur_size, th):
    from shinestacker_amd import NoiseDetection
    assert sum(chunks) == len(frames) and max(chunks) <= NoiseDetection.BATCH == 8
    nd = NoiseDetection(blur_size=blur_size, channel_thresholds=th)
    try:
        at = 0
        for c in chunks:
            nd._device_add(frames[at:at + c])
            at += c
        return nd._device_map(len(frames), frames[0].shape)
    finally:
        nd._release()


def check_noise_detection(frames, chunks, blur_size):
    n = len(frames)
    sums = pr.accumulate(frames)
    th, diff = thresholds_on_the_data(sums, n, blur_size)
    want_mean, want_map, want_counts = pr.hot_map(sums, n, blur_size, th)
    at_least = [int((diff[..., c] >= th[c]).sum()) for c in range(3)]
    assert all(a > b for a, b in zip(at_least, want_counts[1:])), "no pixel sits on a threshold"
    mean, hot, counts = run_noise_detection(frames, chunks, blur_size, th)
    name = (frames[0].shape, n, blur_size, th)
    assert mean.dtype == np.uint8 and np.array_equal(mean, want_mean), name
    assert hot.dtype == np.uint8 and np.array_equal(hot, want_map), name
    assert counts == want_counts, (name, counts, want_counts)
    return want_counts


@pytest.mark.parametrize("h,w", [(5, 7), (2, 3), (3, 2), (1, 5), (16, 16), (32, 48), (17, 33), (75, 101)])
def test_noise_detection_small_frames(dev, h, w):
    """5 x 7 and 2 x 3: smaller than the halo of blur 7 (on an axis of 2 the mirror applies more than once; 3 x 2 has that axis
    the other way, 1 x 5 an axis of one sample), 105 and 18 elements (tails of 1 and 2 for frame_accumulate, one frame per
    launch); 16 x 16 and 32 x 48: whole tiles; 17 x 33: one pixel over; 75 x 101: a tail of 1.  1, 8 (one full batch), 9 and 17
    frames, blur 3 / 5 / 7."""
    assert (h, w) not in ((5, 7), (2, 3), (75, 101)) or (h * w * 3) % 4 == {(5, 7): 1, (2, 3): 2, (75, 101): 1}[(h, w)]
    seen = 0
    for n, chunks in CHUNKS.items():
        frames = noise_frames(h, w, n)
        for blur_size in (3, 5, 7):
            seen += check_noise_detection(frames, chunks, blur_size)[0]
    assert seen > 0


def test_noise_detection_accumulate_goes_round_its_grid(dev):
    """1200 x 1200 x 3 = 4.32 M elements: more than the 4096 x 256 threads x 4 elements of one trip"""
    h = w = 1200
    assert h * w * 3 // 4 > 4096 * 256
    base = noise_frames(h, w, 1)[0]
    frames = [base + np.uint8(3 * f) for f in range(9)]        # wraps modulo 256
    frames[1] = np.full((h, w, 3), 255, np.uint8)
    assert check_noise_detection(frames, CHUNKS[9], 5)[0] > 0


# ---------------------------------------------------------------- radial_ring_sums
def check_ring_sums(lib, img, r_steps, subsample, fast):
    from shinestacker_amd import vignetting as vg
    buf = lib.DeviceBuffer(img.nbytes)
    try:
        buf.upload(img)
        _, means, sums, counts = vg.radial_ring_sums_device(buf.ptr, img.shape[0], img.shape[1], img.dtype, r_steps, subsample, fast)
    finally:
        buf.free()
    want_sums, want_counts = pr.ring_sums(img, r_steps, subsample, fast)
    name = (img.shape, img.dtype, r_steps, subsample, fast)
    assert np.array_equal(counts.astype(np.int64), want_counts), name
    assert np.array_equal(sums.astype(np.int64), want_sums), name
    assert np.array_equal(means, pr.ring_means(want_sums, want_counts), equal_nan=True), name
    return want_counts


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_radial_ring_sums_edges(dev, dtype):
    """r_steps 1 and 2048 (the limits), frames of 1 and 6 pixels, sub-sampling 8 on 9 x 20 (1 x 2 blocks by area, 2 x 3 strided)
    and on 12 x 21 (2 x 3 by area, the last block row and column cut by the frame), area and strided"""
    for h, w in ((1, 1), (2, 3), (203, 301)):
        img = make_frame(h, w, dtype, 61, full_range=True)
        for r_steps in (1, 2, 2048):
            counts = check_ring_sums(dev, img, r_steps, 1, False)
            assert counts.sum() == h * w - 1        # the corner pixel (0, 0) lies at r_max exactly: in no ring
    for h, w in ((9, 20), (12, 21), (37, 53)):
        img = make_frame(h, w, dtype, 67, full_range=True)
        for fast in (False, True):
            for s in (8, 3):
                for r_steps in (1, 7, 2048):
                    check_ring_sums(dev, img, r_steps, s, fast)
    assert pr.subsampled_gray(make_frame(9, 20, dtype, 67), 8, False).shape == (1, 2)
    assert pr.subsampled_gray(make_frame(12, 21, dtype, 67), 8, False).shape == (2, 3)


# ---------------------------------------------------------------- argument checks
def test_entry_points_refuse_bad_arguments(dev):
    """every refusal comes back as the library's message before anything is launched; a good call still works afterwards"""
    from shinestacker_amd import InvalidOptionError
    lib = dev.load()
    buf = dev.DeviceBuffer(1 << 16)
    p, u8, f32 = buf.ptr, dev.DTYPE_CODE[np.dtype(np.uint8)], dev.DTYPE_CODE[np.dtype(np.float32)]
    radii = np.linspace(0, 10, 2050)
    sums, counts = np.zeros(2049, np.uint64), np.zeros(2049, np.uint32)
    th = (C.c_int * 3)(13, 13, 13)
    four = np.zeros(4, np.uint32)

    def ring(img=p, scratch=p + 4096, dtype=u8, r_steps=10, rad=radii.ctypes.data, s=sums.ctypes.data, c=counts.ctypes.data):
        return lib.mi_radial_ring_sums_device(0, None, img, scratch, 8, 8, dtype, 1, 0, r_steps, rad, s, c)

    def vign(src=p, dst=p + 4096, dtype=u8):
        return lib.mi_vignette_apply_device(0, None, src, dst, 8, 8, dtype, 360.0, 0.5, 4.0, 120.0, 1.0, 1.0)

    def mask(src=p, dst=p + 4096, dtype=u8, coords=p + 8192, n=2, ks=3, method=0, stage=p + 8192 + 64):
        return lib.mi_mask_noise_device(0, None, src, dst, 8, 8, dtype, coords, n, ks, method, stage)

    def acc(frames=p, n=1, elements=192, total=p + 4096):
        return lib.mi_frame_accumulate_device(0, None, frames, n, elements, total)

    def hot(total=p, n=1, blur_size=5, thresholds=th, mean=p + 8192, hot_map=p + 12288, dev_counts=p + 16384, out=four.ctypes.data):
        return lib.mi_hot_pixel_map_device(0, None, total, n, 8, 8, blur_size, thresholds, mean, hot_map, dev_counts, out)
    bad = [
        (ring(img=None), "null"), (ring(scratch=None), "null"), (ring(rad=None), "null"), (ring(s=None), "null"), (ring(c=None), "null"),
        (ring(dtype=f32), "dtype"), (ring(r_steps=0), "r_steps"), (ring(r_steps=2049), "r_steps"),
        (vign(src=None), "null"), (vign(dst=None), "null"), (vign(dtype=f32), "dtype"), (vign(src=p + 4), "16-byte aligned"),
        (vign(dst=p + 4096 + 4), "16-byte aligned"),
        (mask(src=None), "null"), (mask(dst=None), "null"), (mask(coords=None), "null"), (mask(stage=None), "null"),
        (mask(dtype=f32), "dtype"), (mask(ks=0), "kernel_size"), (mask(ks=2), "kernel_size"), (mask(ks=4), "kernel_size"),
        (mask(method=2), "method"), (mask(method=-1), "method"),
        (acc(frames=None), "bad argument"), (acc(total=None), "bad argument"), (acc(total=p + 4096 + 4), "aligned"),
        (acc(frames=p + 1), "aligned"), (acc(n=2, elements=6), "aligned"), (acc(n=2, elements=105), "aligned"),
        (hot(total=None), "null"), (hot(thresholds=None), "null"), (hot(hot_map=None), "null"), (hot(dev_counts=None), "null"),
        (hot(out=None), "null"), (hot(n=0), "bad argument"),
    ]
    try:
        for rc, text in bad:
            assert rc != 0, text
        # the message belongs to the last call: ask again one by one
        for call, text in ((lambda: ring(r_steps=2049), "r_steps must be in [1, 2048]"), (lambda: vign(src=p + 4), "16-byte aligned"),
                           (lambda: mask(ks=4), "kernel_size must be odd"), (lambda: mask(method=2), "bad method 2"),
                           (lambda: acc(n=2, elements=6), "sums must be 16-byte aligned, frames 4-byte aligned"),
                           (lambda: hot(n=0), "bad argument"), (lambda: vign(dtype=f32), "dtype must be MI_U8 or MI_U16")):
            with pytest.raises(ValueError) as err:
                dev.check(call())
            assert text in str(err.value)
        with pytest.raises(InvalidOptionError, match="blur_size must be 3, 5 or 7"):
            dev.check(hot(blur_size=9))
        # one odd-sized frame alone needs no whole dwords; the calls above left nothing behind
        frame = np.arange(105, dtype=np.uint8)
        buf.upload(frame)
        buf.upload(np.zeros(105, np.uint32), 4096)
        dev.check(acc(n=1, elements=105))
        sync(dev)
        assert np.array_equal(buf.download((105,), np.uint32, 4096), frame)
    finally:
        buf.free()
