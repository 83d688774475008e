"""CPU: the depth-selected composite's restatement (tests/depth_render_restatement.py) against hand-computed pixels and its own
chunked form, and every refusal of depth_render.check_options, pipeline._check_brush with "depth_composite" and the
depth_composite= dict."""
import numpy as np
import pytest

import depth_render_restatement as dr
from shinestacker_amd import InvalidOptionError, Stroke, depth_render, pipeline


def stack_of(values, dtype):
    """N frames of one pixel, frame i holding values[i] in channel 0, values[i] with the sign of the type's zero in 1, 2"""
    return [np.full((1, 1, 3), v, dtype) for v in values]


def plane(*d):
    return np.array([d], np.float32)


def row(frames, depth, interp):
    """the composite of one-pixel frames over a row of depths: channel 0 of every pixel"""
    w = depth.shape[1]
    wide = [np.repeat(np.asarray(fr), w, axis=1) for fr in frames]
    return dr.composite(wide, depth, interp)[0, :, 0]


def test_nearest_rounds_ties_to_even():
    fr = stack_of([10, 20, 30, 40], np.uint8)
    got = row(fr, plane(0.5, 1.5, 2.5, 0.49, 0.51, 3.0), "nearest")
    assert got.tolist() == [10, 30, 30, 10, 20, 40]         # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2


def test_linear_by_hand():
    fr = stack_of([10, 20, 30, 41], np.uint8)
    # 0.25: 10 + 0.25 * 10 = 12.5 -> 12 (even); 0.75: 17.5 -> 18; 2.5: 30 + 5.5 = 35.5 -> 36; 1.0: f == 0 -> 20
    got = row(fr, plane(0.25, 0.75, 2.5, 1.0), "linear")
    assert got.tolist() == [12, 18, 36, 20]
    hi = stack_of([65535, 0, 65535], np.uint16)
    assert row(hi, plane(0.5, 1.5, 0.0, 2.0), "linear").tolist() == [32768, 32768, 65535, 65535]    # 32767.5 -> 32768 (even)


@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_the_ends_of_the_stack(interp):
    fr = stack_of([10, 20, 30, 40], np.uint16)
    # d = N - 1 exactly: k0 = 3 = k1, f = 0; below 0, above N - 1, NaN -> 0, -inf, +inf
    got = row(fr, plane(3.0, -0.5, -7.0, 3.5, 100.0, np.nan, -np.inf, np.inf), interp)
    assert got.tolist() == [40, 10, 10, 40, 40, 10, 10, 40]
    _, k0, f, k1, k = dr.indices(plane(3.0, np.nan, 9.0), 4)
    assert k0.tolist() == [[3, 0, 3]] and k1.tolist() == [[3, 1, 3]] and f.tolist() == [[0.0, 0.0, 0.0]] and k.tolist() == [[3, 0, 3]]


@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_a_single_frame(interp, dtype):
    rng = np.random.default_rng(1)
    fr = (rng.random((4, 5, 3)) * 200).astype(dtype)
    depth = np.array(rng.random((4, 5)) * 6 - 3, np.float32)
    depth[0, 0] = np.nan
    assert np.array_equal(dr.composite([fr], depth, interp), fr)
    assert dr.chunks(1, 2) == [(0, 1)]


def test_a_zero_fraction_selects_the_sample_bit_for_bit():
    """float32 frames with negative, fractional and signed-zero samples beside a neighbour that would spoil a computed result:
    a + 0 * (b - a) turns -0 into +0 and an infinite b - a into NaN"""
    a = np.array([[[-0.0, -1.5e-7, 3.0e38]], [[-123.456, 0.1, -3.0e38]]], np.float32)
    b = np.array([[[5.0, 1.0e6, -3.0e38]], [[np.inf, -0.3, 3.0e38]]], np.float32)
    c = np.array([[[7.25, -7.25, 1.0]], [[-0.0, 2.5, -1.0e6]]], np.float32)
    depth = np.array([[0.0], [1.0]], np.float32)
    got = dr.composite([a, b, c], depth, "linear")
    assert got[0].tobytes() == a[0].tobytes() and got[1].tobytes() == b[1].tobytes()
    depth = np.array([[2.0], [-3.0]], np.float32)           # the k1 clamp and the lower clamp: f == 0 again
    got = dr.composite([a, b, c], depth, "linear")
    assert got[0].tobytes() == c[0].tobytes() and got[1].tobytes() == a[1].tobytes()
    # a computed sample: one subtract, one multiply, one add, each rounded to float32
    d = np.float32(0.3)
    depth = np.array([[d], [d]], np.float32)
    got = dr.composite([a, c], depth, "linear")
    want = (a + (d * (c - a).astype(np.float32)).astype(np.float32)).astype(np.float32)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_identical_frames_come_back_for_any_depth(interp, dtype):
    rng = np.random.default_rng(2)
    if dtype == np.float32:
        fr = ((rng.random((6, 9, 3)) - 0.5) * 2.0e6).astype(np.float32)
    else:
        fr = rng.integers(0, np.iinfo(dtype).max + 1, (6, 9, 3)).astype(dtype)
    depth = np.array(rng.random((6, 9)) * 7 - 1, np.float32)
    depth[1, 1], depth[2, 2], depth[3, 3] = np.nan, 0.5, 4.0
    assert np.array_equal(dr.composite([fr] * 5, depth, interp), fr)


def cases(n, shape=(7, 11), seed=3):
    rng = np.random.default_rng(seed)
    u8 = [rng.integers(0, 256, shape + (3,)).astype(np.uint8) for _ in range(n)]
    u16 = [rng.integers(0, 65536, shape + (3,)).astype(np.uint16) for _ in range(n)]
    f32 = [((rng.random(shape + (3,)) - 0.5) * 2.0e6).astype(np.float32) for _ in range(n)]
    depth = np.array(rng.random(shape) * (n + 1) - 1, np.float32)
    depth.flat[::7] = np.nan
    depth.flat[1::9] = np.arange(depth.flat[1::9].size) % n              # whole indices, the last frame among them
    depth.flat[2::9] = (np.arange(depth.flat[2::9].size) % n) + 0.5      # ties
    return {"u8": u8, "u16": u16, "f32": f32}, depth


@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("n", [2, 5, 6])
def test_the_chunks_give_the_whole(interp, n):
    stacks, depth = cases(n)
    for name, fr in stacks.items():
        whole = dr.composite(fr, depth, interp)
        for size in (2, 3, n):
            sentinel = 77
            got = dr.composite_chunked(fr, depth, size, interp, fill=sentinel)
            assert got.tobytes() == whole.tobytes(), (name, size)
        # every pixel belongs to exactly one call
        _, k0, _, _, _ = dr.indices(depth, n)
        hits = sum(dr.owned(k0, first, count, n).astype(int) for first, count in dr.chunks(n, 3))
        assert (hits == 1).all()


def test_a_middle_chunk_owns_only_its_pixels():
    stacks, depth = cases(6)
    fr = stacks["u16"]
    out = np.full_like(fr[0], 4242)
    dr.composite_chunk(fr[2:4], 2, 6, depth, out, "linear")
    _, k0, _, _, _ = dr.indices(depth, 6)
    mine = k0 == 2
    assert mine.any() and not mine.all()
    assert (out[~mine] == 4242).all() and np.array_equal(out[mine], dr.composite(fr, depth, "linear")[mine])


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", ["cubic", "", None, 0, 1, True, b"linear", ["linear"]])
def test_check_options_refuses(bad):
    with pytest.raises(InvalidOptionError):
        depth_render.check_options(bad)


def test_check_options_accepts():
    assert depth_render.check_options() == "linear" and depth_render.check_options("nearest") == "nearest"
    assert depth_render.INTERP == {"linear": 0, "nearest": 1}


@pytest.mark.parametrize("first, count, n", [(0, 0, 3), (-1, 2, 3), (2, 2, 3), (0, 4, 3), (1, 1, 3), (0, 1, 0), (0, 2.0, 3), (True, 2, 3)])
def test_check_chunk_refuses(first, count, n):
    with pytest.raises(InvalidOptionError):
        depth_render.check_chunk(first, count, n)


def test_check_chunk_accepts():
    for first, count, n in [(0, 1, 1), (0, 2, 2), (1, 2, 3), (0, 3, 3), (38, 2, 40)]:
        depth_render.check_chunk(first, count, n)


def test_composite_checks_its_arguments_before_it_needs_a_device():
    from shinestacker_amd import BitDepthError, ShapeError
    fr = np.zeros((4, 6, 3), np.uint8)
    d = np.zeros((4, 6), np.float32)
    with pytest.raises(InvalidOptionError):
        depth_render.composite([fr, fr], d, interp="cubic")
    with pytest.raises(InvalidOptionError):
        depth_render.composite([fr, fr], d, resident=1)
    with pytest.raises(InvalidOptionError):
        depth_render.composite([fr, fr], np.zeros((4, 5), np.float32))
    with pytest.raises(InvalidOptionError):
        depth_render.composite([np.zeros((4, 6), np.uint8)], d)
    with pytest.raises(BitDepthError):
        depth_render.composite([fr.astype(np.int16)], d)
    with pytest.raises(ValueError):
        depth_render.composite(iter(()), d)
    with pytest.raises(BitDepthError):
        depth_render.composite_device([1, 2], 0, 2, 2, 3, 4, 4, 6, np.float64)
    with pytest.raises(InvalidOptionError):
        depth_render.composite_device([1, 2, 3], 0, 2, 2, 3, 4, 4, 6, np.uint8)
    # a later frame of another type or shape is refused by the reader (it needs the device only to get that far)
    assert issubclass(ShapeError, Exception)


def test_check_brush_takes_the_composite_only_when_it_is_on():
    s = Stroke("depth_composite", [(1, 1)], 11)
    with pytest.raises(InvalidOptionError):
        pipeline._check_brush([s], 3)
    with pytest.raises(InvalidOptionError):
        pipeline._check_brush([s], 3, None)
    opts = pipeline._check_depth_composite({}, {}, (40, 60), None)
    assert pipeline._check_brush([s, Stroke(2, [(1, 1)], 11)], 3, opts)[0] is s
    for other in ("depth_composit", "frame.jpg"):
        with pytest.raises(InvalidOptionError):
            pipeline._check_brush([Stroke(other, [(1, 1)], 11)], 3, opts)
    with pytest.raises(InvalidOptionError):
        pipeline._check_brush([Stroke(3, [(1, 1)], 11)], 3, opts)


def test_depth_composite_dict():
    from shinestacker_amd import depth_out
    assert pipeline._check_depth_composite(None, None, (40, 60), None) is None
    assert pipeline._check_depth_composite({}, {}, (40, 60), None) == {"interp": "linear", "sigma": depth_out.PYRAMID_SIGMA}
    assert pipeline._check_depth_composite({}, {}, (40, 60), 3.0)["sigma"] == 3.0
    assert pipeline._check_depth_composite({"sigma": 0, "interp": "nearest"}, {}, (40, 60), 3.0) == {"interp": "nearest", "sigma": 0.0}
    for bad in ({"interpolation": "linear"}, {"interp": "cubic"}, {"sigma": -1}, {"sigma": 17}, {"sigma": 16}, 5, "linear"):
        with pytest.raises(InvalidOptionError):
            pipeline._check_depth_composite(bad, {}, (40, 60), None)
    with pytest.raises(InvalidOptionError):
        pipeline._check_depth_composite({}, None, (40, 60), None)       # no info dict to return it in


def test_pipeline_refuses_before_it_needs_a_device():
    fr = [np.zeros((40, 60, 3), np.uint8)] * 3
    with pytest.raises(InvalidOptionError):
        pipeline.align_and_stack(fr, depth_composite={"interp": "cubic"}, info={})
    with pytest.raises(InvalidOptionError):
        pipeline.align_and_stack(fr, depth_composite={})
    with pytest.raises(InvalidOptionError):
        pipeline.align_and_stack(fr, retouch=[Stroke("depth_composite", [(1, 1)], 11)])
    with pytest.raises(InvalidOptionError):
        pipeline.align_and_stack_device(0, 3, 40, 60, np.uint8, depth_composite={"key": 1}, info={})


def test_actions_refuse():
    from shinestacker_amd import FocusStack, FocusStackBunch, PyramidStack
    from shinestacker_amd.pyramid import BaseStackAlgo

    class NoDepth(BaseStackAlgo):
        def __init__(self):
            super().__init__("nodepth", 1)
    with pytest.raises(InvalidOptionError):
        FocusStack("s", PyramidStack(), depth_composite_path="dc", depth_composite_interp="cubic")
    with pytest.raises(InvalidOptionError):
        FocusStackBunch("s", PyramidStack(), depth_composite_path="dc", depth_map_sigma=99)
    with pytest.raises(InvalidOptionError):
        FocusStack("s", PyramidStack(), retouch=[Stroke("depth_composite", [(1, 1)], 11)])
    with pytest.raises(InvalidOptionError):
        FocusStack("s", NoDepth(), depth_composite_path="dc")
    a = FocusStack("s", PyramidStack(), depth_composite_path="dc", retouch=[Stroke("depth_composite", [(1, 1)], 11)])
    assert a.depth_composite_path == "dc" and a.depth_composite_interp == "linear"
    assert FocusStack("s", PyramidStack()).depth_composite_path is None


def test_the_abi_refuses_before_any_device_call(hiplib):
    """null pointers, a bad chunk, an unknown dtype or interp, and an output that aliases a frame: MI_ERR_INVALID, on a machine
    without a GPU too"""
    import ctypes as C
    lib = hiplib.load()
    fr = [np.zeros((4, 8, 3), np.uint8) for _ in range(3)]
    depth = np.zeros((4, 8), np.float32)
    out = np.zeros((4, 8, 3), np.uint8)
    tab = (C.c_void_p * 3)(*[f.ctypes.data for f in fr])

    def dev(t=tab, first=0, count=3, n=3, d=depth.ctypes.data, o=out.ctypes.data, h=4, w=8, dt=hiplib.MI_U8, interp=0):
        return lib.mi_depth_composite_device(0, None, t, first, count, n, d, o, h, w, dt, interp)

    def host(t=tab, first=0, count=3, n=3, d=depth.ctypes.data, o=out.ctypes.data, h=4, w=8, dt=hiplib.MI_U8, interp=0):
        return lib.mi_depth_composite(0, t, first, count, n, d, o, h, w, dt, interp)
    for call in (dev, host):
        assert call(t=None) == hiplib.MI_ERR_INVALID and b"null" in lib.mi_last_error()
        assert call(d=None) == hiplib.MI_ERR_INVALID and call(o=None) == hiplib.MI_ERR_INVALID
        assert call(count=0) == hiplib.MI_ERR_INVALID
        assert call(first=1) == hiplib.MI_ERR_INVALID and call(first=-1, count=2) == hiplib.MI_ERR_INVALID
        assert call(first=1, count=1) == hiplib.MI_ERR_INVALID
        assert call(dt=hiplib.MI_F64) == hiplib.MI_ERR_INVALID and call(dt=9) == hiplib.MI_ERR_INVALID
        assert call(interp=2) == hiplib.MI_ERR_INVALID and call(interp=-1) == hiplib.MI_ERR_INVALID
        assert call(h=0) == hiplib.MI_ERR_INVALID
        assert call(o=fr[1].ctypes.data) == hiplib.MI_ERR_INVALID and b"alias" in lib.mi_last_error()
        assert call(o=fr[2].ctypes.data + 4) == hiplib.MI_ERR_INVALID and b"alias" in lib.mi_last_error()
        assert call(t=(C.c_void_p * 3)(fr[0].ctypes.data, None, fr[2].ctypes.data)) == hiplib.MI_ERR_INVALID
