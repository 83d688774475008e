"""GPU: a host form returns exactly the bytes its device form returns.

Every feature of the C boundary that takes host arrays (mi_warp_affine, mi_histogram, ...) uploads them, runs the `_device`
entry point and downloads the result.  Here each pair runs side by side on the same seeded inputs: the host form, and the
device form driven by hand (mi_device_malloc, mi_memcpy_h2d, the `_device` call on the null stream, mi_device_synchronize,
mi_memcpy_d2h, mi_device_free -- what _lib.DeviceBuffer wraps).  Both run the same kernel, so every comparison is
np.array_equal with no tolerance.  Each form runs twice in a row and must repeat itself (a buffer reused before its reader
finished would not), and the host form runs again with host_src == host_dst where the entry point allows it.

Shapes: 12 x 16, and 13 x 7 -- odd sides, a width no multiple of 4, narrower than every tile."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(12, 16), (13, 7)]
DTYPES = [np.uint8, np.uint16]
shape_dtype = pytest.mark.parametrize("shape,dtype", [(s, d) for s in SHAPES for d in DTYPES],
                                      ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else np.dtype(v).name)


@pytest.fixture(scope="module")
def lib(hiplib):
    hiplib.require_device()
    return hiplib.load()


def frame(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:       # not small integers: negative, fractional
        return ((rng.random(shape + (3,)) - 0.5) * 2.0e3).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape + (3,)).astype(dtype)


class Device:
    """device buffers for one hand-driven call, freed on the way out"""

    def __init__(self, hiplib):
        self.hiplib, self.bufs = hiplib, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()

    def empty(self, nbytes):
        self.bufs.append(self.hiplib.DeviceBuffer(nbytes))
        return self.bufs[-1]

    def put(self, arr):
        b = self.empty(arr.nbytes)
        b.upload(arr)
        return b

    def sync(self):
        self.hiplib.check(self.hiplib.load().mi_device_synchronize(0))


def same(host, device):
    """run both forms twice: each repeats itself, and the host form equals the device form"""
    h1, d1, h2, d2 = host(), device(), host(), device()
    for a, b, c, d in zip(h1, h2, d1, d2):
        assert np.array_equal(a, b), "the host form does not repeat itself"
        assert np.array_equal(c, d), "the device form does not repeat itself"
        assert a.dtype == c.dtype and a.shape == c.shape and np.array_equal(a, c), "host form != device form"
    return h1


# ------------------------------------------------------------------------------------------------------------ warp
AFFINE = np.array([[1.01, 0.02, 0.7], [-0.015, 0.99, -0.4]], np.float64)
PERSPECTIVE = np.array([[1.01, 0.02, 0.7], [-0.015, 0.99, -0.4], [1.0e-3, -5.0e-4, 1.0]], np.float64)


@shape_dtype
@pytest.mark.parametrize("persp", [False, True], ids=["affine", "perspective"])
def test_warp(hiplib, lib, shape, dtype, persp):
    h, w = shape
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    src = frame(shape, dtype, 1)
    m = np.ascontiguousarray(PERSPECTIVE if persp else AFFINE).ctypes.data_as(C.POINTER(C.c_double))
    bv = (C.c_double * 4)(10.0, 20.0, 30.0, 0.0)
    host_fn = lib.mi_warp_perspective if persp else lib.mi_warp_affine
    dev_fn = lib.mi_warp_perspective_device if persp else lib.mi_warp_affine_device
    for border in (hiplib.BORDER_CONSTANT, hiplib.BORDER_REPLICATE, hiplib.BORDER_REPLICATE_BLUR):
        def host(alias=False):
            a = src.copy()
            out, mask = (a if alias else np.empty_like(a)), np.empty(shape, np.uint8)
            hiplib.check(host_fn(0, a.ctypes.data, out.ctypes.data, mask.ctypes.data, h, w, code, m, border, bv, 5, 2.0))
            return out, mask

        def device():
            with Device(hiplib) as d:
                s, dst, tmp, mask = d.put(src), d.empty(src.nbytes), d.empty(src.nbytes), d.empty(h * w)
                hiplib.check(dev_fn(0, None, s.ptr, dst.ptr, tmp.ptr, mask.ptr, h, w, code, m, border, bv, 5, 2.0))
                d.sync()
                return dst.download(src.shape, dtype), mask.download(shape, np.uint8)

        want = same(host, device)
        for a, b in zip(host(alias=True), want):
            assert np.array_equal(a, b), "host_src == host_dst"


# ------------------------------------------------------------------------------------------- histogram, LUT, colour
@shape_dtype
def test_histogram(hiplib, lib, shape, dtype):
    h, w = shape
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    nbins = 256 if dtype == np.uint8 else 65536
    img = frame(shape, dtype, 2)
    for mode, subsample, fast, mask_size in ((0, 1, 1, 0.0), (1, 1, 1, 0.0), (0, 2, 1, 0.0), (0, 2, 0, 0.0), (1, 1, 1, 0.8)):
        nch = 3 if mode == 0 else 1

        def host():
            counts = np.full((nch, nbins), -1, np.int64)
            hiplib.check(lib.mi_histogram(0, img.ctypes.data, h, w, code, mode, subsample, fast, mask_size, counts.ctypes.data))
            return (counts,)

        def device():
            counts = np.full((nch, nbins), -1, np.int64)
            with Device(hiplib) as d:
                s, scratch = d.put(img), d.empty(3 * nbins * 4)
                hiplib.check(lib.mi_histogram_device(0, None, s.ptr, scratch.ptr, h, w, code, mode, subsample, fast, mask_size,
                                                     counts.ctypes.data))
                d.sync()
            return (counts,)

        (counts,) = same(host, device)
        if subsample == 1 and mask_size == 0.0:
            assert (counts.sum(axis=1) == h * w).all()


@shape_dtype
@pytest.mark.parametrize("nlut", [1, 3])
def test_lut(hiplib, lib, shape, dtype, nlut):
    h, w = shape
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    nbins = 256 if dtype == np.uint8 else 65536
    src = frame(shape, dtype, 3)
    lut = np.random.default_rng(30 + nlut).integers(0, nbins, (nlut, nbins)).astype(dtype)

    def host(alias=False):
        a = src.copy()
        out = a if alias else np.empty_like(a)
        hiplib.check(lib.mi_apply_lut(0, a.ctypes.data, out.ctypes.data, h, w, code, lut.ctypes.data, nlut))
        return (out,)

    def device():
        with Device(hiplib) as d:
            s, dst, t = d.put(src), d.empty(src.nbytes), d.put(lut)
            hiplib.check(lib.mi_apply_lut_device(0, None, s.ptr, dst.ptr, h * w, code, t.ptr, nlut))
            d.sync()
            return (dst.download(src.shape, dtype),)

    (want,) = same(host, device)
    assert np.array_equal(host(alias=True)[0], want), "host_src == host_dst"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("code", [0, 1, 2, 3], ids=["bgr2hsv", "hsv2bgr", "bgr2hls", "hls2bgr"])
def test_cvt_color(hiplib, lib, shape, code):
    h, w = shape
    src = frame(shape, np.uint8, 4)

    def host(alias=False):
        a = src.copy()
        out = a if alias else np.empty_like(a)
        hiplib.check(lib.mi_cvt_color(0, a.ctypes.data, out.ctypes.data, h, w, hiplib.MI_U8, code))
        return (out,)

    def device():       # in place, as the host form runs it
        with Device(hiplib) as d:
            s = d.put(src)
            hiplib.check(lib.mi_cvt_color_device(0, None, s.ptr, s.ptr, h * w, hiplib.MI_U8, code))
            d.sync()
            return (s.download(src.shape, np.uint8),)

    (want,) = same(host, device)
    assert np.array_equal(host(alias=True)[0], want), "host_src == host_dst"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cvt_color_is_8_bit_only_in_both_forms(hiplib, lib, shape):
    h, w = shape
    src = frame(shape, np.uint16, 4)
    out = np.empty_like(src)
    assert lib.mi_cvt_color(0, src.ctypes.data, out.ctypes.data, h, w, hiplib.MI_U16, 0) == hiplib.MI_ERR_UNSUPPORTED
    with Device(hiplib) as d:
        s = d.put(src)
        assert lib.mi_cvt_color_device(0, None, s.ptr, s.ptr, h * w, hiplib.MI_U16, 0) == hiplib.MI_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------ denoise, unsharp mask
@shape_dtype
def test_nlm_denoise(hiplib, lib, shape, dtype):
    from shinestacker_amd.denoise import weight_table
    h, w = shape
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    src = frame(shape, dtype, 5)
    tw, sw = 3, 5           # inside MI_NLM_MAX_*; the reflected border of 3 pixels stays below both sides
    table, shift = weight_table(dtype, 40 if dtype == np.uint8 else 40 * 256, tw, sw)
    args = (h, w, code, table.ctypes.data, int(table.size), int(shift), tw, sw)

    def host(alias=False):
        a = src.copy()
        out = a if alias else np.empty_like(a)
        hiplib.check(lib.mi_nlm_denoise(0, a.ctypes.data, out.ctypes.data, *args))
        return (out,)

    def device():
        with Device(hiplib) as d:
            s, dst = d.put(src), d.empty(src.nbytes)
            hiplib.check(lib.mi_nlm_denoise_device(0, s.ptr, dst.ptr, *args, None))
            d.sync()
            return (dst.download(src.shape, dtype),)

    (want,) = same(host, device)
    assert not np.array_equal(want, src)
    assert np.array_equal(host(alias=True)[0], want), "host_src == host_dst"


@shape_dtype
@pytest.mark.parametrize("threshold", [0.0, 3.0])
def test_unsharp_mask(hiplib, lib, shape, dtype, threshold):
    from shinestacker_amd.sharpen import _prepare
    h, w = shape
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    src = frame(shape, dtype, 6)
    taps, ksize, amount, thr = _prepare(dtype, 1.0, 1.5, threshold)

    def host(alias=False):
        a = src.copy()
        out = a if alias else np.empty_like(a)
        hiplib.check(lib.mi_unsharp_mask(0, a.ctypes.data, out.ctypes.data, h, w, code, taps.ctypes.data, ksize, amount, thr))
        return (out,)

    def device():
        with Device(hiplib) as d:
            s, dst = d.put(src), d.empty(src.nbytes)
            hiplib.check(lib.mi_unsharp_mask_device(0, None, s.ptr, dst.ptr, h, w, code, taps.ctypes.data, ksize, amount, thr))
            d.sync()
            return (dst.download(src.shape, dtype),)

    (want,) = same(host, device)
    assert not np.array_equal(want, src)
    assert np.array_equal(host(alias=True)[0], want), "host_src == host_dst"


# ------------------------------------------------------------------------------------------------------ stereo view
@shape_dtype
@pytest.mark.parametrize("shift", [2.5, -6.0])
def test_stereo_view(hiplib, lib, shape, dtype, shift):
    h, w = shape
    assert int(np.ceil(abs(shift))) < w
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    n_frames = 5
    img = frame(shape, dtype, 7)
    depth = (np.random.default_rng(70).random(shape) * (n_frames - 1)).astype(np.float32)
    args = (h, w, code, n_frames, shift, 0.4, 1)

    def host(alias=False):
        a = img.copy()
        out = a if alias else np.empty_like(a)
        hiplib.check(lib.mi_stereo_view(0, a.ctypes.data, depth.ctypes.data, out.ctypes.data, *args))
        return (out,)

    def device():
        with Device(hiplib) as d:
            s, dep, dst = d.put(img), d.put(depth), d.empty(img.nbytes)
            hiplib.check(lib.mi_stereo_view_device(0, None, s.ptr, dep.ptr, dst.ptr, *args))
            d.sync()
            return (dst.download(img.shape, dtype),)

    (want,) = same(host, device)
    assert not np.array_equal(want, img)
    assert np.array_equal(host(alias=True)[0], want), "host_img == host_out"


# ---------------------------------------------------------------------------------------------- brush stroke, blend
@shape_dtype
def test_brush_stroke_with_mask(hiplib, lib, shape, dtype):
    from shinestacker_amd import retouch
    h, w = shape
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    master, source = frame(shape, dtype, 8), frame(shape, dtype, 9)
    radius, opacity = 3, 0.8
    table = retouch._stamp_table(radius, 40, 80, 70)
    stamps = np.array([(2, 3), (4, 4), (w - 1, h - 2), (4, 4), (-50, -50), (w + 1, 0)], np.int32)
    box = np.asarray(retouch.stroke_box(stamps, radius, h, w), np.int32)
    assert box[0] < box[2]

    def host():
        out, mask, area = master.copy(), np.full(shape, -1.0, np.float64), np.full(4, -1, np.int32)
        hiplib.check(lib.mi_brush_stroke(0, out.ctypes.data, source.ctypes.data, h, w, code, table.ctypes.data, radius,
                                         stamps.ctypes.data, len(stamps), opacity, mask.ctypes.data, area.ctypes.data))
        return out, mask, area

    def device():
        with Device(hiplib) as d:
            m, s, t, st, mask = d.put(master), d.put(source), d.put(table), d.put(stamps), d.empty(h * w * 8)
            hiplib.check(lib.mi_brush_stroke_device(0, None, m.ptr, s.ptr, h, w, code, t.ptr, radius, st.ptr, len(stamps),
                                                    box.ctypes.data, opacity, mask.ptr))
            d.sync()
            return m.download(master.shape, dtype), mask.download(shape, np.float64), box

    out, mask, _ = same(host, device)
    assert not np.array_equal(out, master) and mask.max() > 0


def test_a_stroke_that_misses_the_frame_paints_nothing(hiplib, lib):
    """the host form returns before it touches the device: the master stays, the mask is zeroed, the area is empty"""
    from shinestacker_amd import retouch
    shape = (13, 7)
    master, source = frame(shape, np.uint8, 8), frame(shape, np.uint8, 9)
    table = retouch._stamp_table(3, 40, 80, 70)
    stamps = np.array([(-50, -50), (100, 3)], np.int32)
    out, mask, area = master.copy(), np.full(shape, -1.0, np.float64), np.full(4, -1, np.int32)
    hiplib.check(lib.mi_brush_stroke(0, out.ctypes.data, source.ctypes.data, 13, 7, hiplib.MI_U8, table.ctypes.data, 3,
                                     stamps.ctypes.data, len(stamps), 0.8, mask.ctypes.data, area.ctypes.data))
    assert np.array_equal(out, master) and not mask.any() and not area.any()


@shape_dtype
def test_blend_mask(hiplib, lib, shape, dtype):
    h, w = shape
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    master, source = frame(shape, dtype, 10), frame(shape, dtype, 11)
    mask = np.random.default_rng(110).random(shape)

    def host():
        out = master.copy()
        hiplib.check(lib.mi_blend_mask(0, out.ctypes.data, source.ctypes.data, mask.ctypes.data, h, w, code, 0.9))
        return (out,)

    def device():
        with Device(hiplib) as d:
            m, s, k = d.put(master), d.put(source), d.put(mask)
            hiplib.check(lib.mi_blend_mask_device(0, None, m.ptr, s.ptr, k.ptr, h, w, code, 0.9))
            d.sync()
            return (m.download(master.shape, dtype),)

    (out,) = same(host, device)
    assert not np.array_equal(out, master)


# ------------------------------------------------------------------------------------------------ depth composite
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES + [np.float32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "nearest"])
def test_depth_composite(hiplib, lib, shape, dtype, interp):
    """a middle chunk of the stack: the pixels of the other chunks keep what host_out held"""
    h, w = shape
    code = hiplib.DTYPE_CODE[np.dtype(dtype)]
    n_frames, first, count = 5, 1, 3
    frames = [frame(shape, dtype, 120 + i) for i in range(count)]
    held = frame(shape, dtype, 12)
    depth = (np.random.default_rng(121).random(shape) * (n_frames + 1) - 1).astype(np.float32)
    depth[0, 0] = np.nan

    def host():
        out = held.copy()
        ptrs = (C.c_void_p * count)(*[f.ctypes.data for f in frames])
        hiplib.check(lib.mi_depth_composite(0, ptrs, first, count, n_frames, depth.ctypes.data, out.ctypes.data, h, w, code, interp))
        return (out,)

    def device():
        with Device(hiplib) as d:
            bufs, dep, out = [d.put(f) for f in frames], d.put(depth), d.put(held)
            ptrs = (C.c_void_p * count)(*[b.ptr for b in bufs])
            hiplib.check(lib.mi_depth_composite_device(0, None, ptrs, first, count, n_frames, dep.ptr, out.ptr, h, w, code, interp))
            d.sync()
            return (out.download(held.shape, dtype),)

    (out,) = same(host, device)
    changed = (out != held).any(axis=2)
    assert changed.any() and not changed.all()


# ------------------------------------------------------------------------ weighted smoothing, the stack's depth map
@pytest.mark.parametrize("shape,min_size", [((12, 16), 4), ((13, 7), 2)], ids=["12x16", "13x7"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_stack_depth_map_and_weighted_smooth(hiplib, lib, shape, min_size, dtype):
    """mi_stack_depth_map against mi_stack_depth_map_device, and mi_weighted_smooth on the planes the stack smooths (its
    level-0 winner index and energy) against both: three ways into the same kernels"""
    from shinestacker_amd import depth_out
    h, w = shape
    with hiplib.Stack(h, w, in_dtype=dtype, min_size=min_size) as st:
        assert st.levels >= 1
        for i in range(3):
            st.push_frame(frame(shape, dtype, 130 + i))
        st.sync()
        index, energy = st.tap(hiplib.TAP_INDEX, 0), st.tap(hiplib.TAP_ENERGY, 0)
        for sigma in (0.0, 1.0):
            assert depth_out.radius_of(sigma) < min(h, w)

            def host():
                return (st.depth_map(sigma),)

            def device():
                with Device(hiplib) as d:
                    out = d.empty(h * w * 4)
                    st.depth_map(sigma, dev_ptr=out.ptr)
                    return (out.download(shape, np.float32),)

            (want,) = same(host, device)
            for _ in range(2):
                got = depth_out.weighted_smooth(index, energy, sigma)
                assert got.dtype == want.dtype and np.array_equal(got, want), "mi_weighted_smooth != mi_stack_depth_map"
            if sigma > 0:     # the value plane may be the output plane: both are 4-byte planes, uploaded before any download
                v = energy.copy()
                hiplib.check(lib.mi_weighted_smooth(0, v.ctypes.data, energy.ctypes.data, h, w, 0, hiplib.MI_F32, sigma, v.ctypes.data))
                assert np.array_equal(v, depth_out.weighted_smooth(energy, energy, sigma)), "host_value == host_out"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_weighted_smooth_float64(hiplib, lib, shape):
    """the float-64 working type has no cheap stack behind it: the host form repeats itself, and without smoothing it
    returns the value plane"""
    from shinestacker_amd import depth_out
    rng = np.random.default_rng(14)
    value, weight = rng.integers(0, 9, shape).astype(np.int32), rng.random(shape)
    a, b = depth_out.weighted_smooth(value, weight, 1.0), depth_out.weighted_smooth(value, weight, 1.0)
    assert a.dtype == np.float32 and np.array_equal(a, b) and not np.array_equal(a, value)
    for _ in range(2):
        assert np.array_equal(depth_out.weighted_smooth(value, weight, 0.0), value.astype(np.float32))
