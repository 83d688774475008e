"""CPU: the stereo view's specification as tests/stereo_restatement.py states it (translation, occlusion, hole filling,
near='first', clamping, the pair layouts, the rocking shifts), and what shinestacker_amd.stereo, the C entry points and the
actions decide without a device (option checks, MI_ERR_INVALID, the stacker without a depth map)."""
import inspect

import numpy as np
import pytest

import stereo_restatement as sr
from shinestacker_amd import DeviceError, InvalidOptionError, stereo


def image(shape, dtype=np.uint8, seed=1):
    """every pixel distinct enough to tell which source column it came from"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape + (3,)).astype(dtype)


def from_columns(img, xs):
    """out[y, x'] = img[y, xs[x']] for one list of source columns shared by every row"""
    return img[:, np.asarray(xs)]


# ------------------------------------------------------------------ the specification, on the restatement
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_shift_zero_returns_the_image(dtype):
    img = image((6, 31), dtype)
    depth = np.random.default_rng(2).random((6, 31)).astype(np.float32) * 7
    for near in ("last", "first"):
        out = sr.view(img, depth, 8, 0.0, 0.3, near)
        assert out.dtype == img.dtype and np.array_equal(out, img)


@pytest.mark.parametrize("shift,z,pivot", [(12.0, 6.0, 0.5), (-12.0, 6.0, 0.5), (7.0, 0.0, 1.0), (64.0, 8.0, 0.0), (16.0, 2.0, 0.75),
                                           (-9.0, 8.0, 0.75)])
def test_a_flat_depth_plane_is_a_translation(shift, z, pivot):
    """every source has one t, so d = rint(shift * (t - pivot)) for all: out[x'] = img[x' - d], and the d columns nothing
    lands on, at one edge, have a filled neighbour on one side only: the edge column of the image"""
    n, w = 9, 80                                    # t = z / 8: exact
    img = image((4, w))
    d = int(np.rint(np.float32(shift) * (np.float32(z / 8.0) - np.float32(pivot))))
    assert d == round(shift * (z / 8.0 - pivot)) and d != 0        # the cases are exact products, no halves
    out = sr.view(img, np.full((4, w), z, np.float32), n, shift, pivot)
    assert np.array_equal(out, from_columns(img, np.clip(np.arange(w) - d, 0, w - 1)))
    if d > 0:
        assert np.array_equal(out[:, :d], np.repeat(img[:, :1], d, axis=1))
    else:
        assert np.array_equal(out[:, w + d:], np.repeat(img[:, -1:], -d, axis=1))


def test_two_plateaus_occlude_on_one_side_and_open_a_hole_on_the_other():
    n, w, c = 5, 40, 17                             # far plateau (frame 0, t = 0) left of column c, near plateau (t = 1) from c on
    img = image((3, w))
    depth = np.zeros((3, w), np.float32)
    depth[:, c:] = n - 1
    # shift +8, pivot 0.5: far moves by -4, near by +4 -- they part.  Far lands on [.., c - 5], near on [c + 4, ..]; the 8
    # targets between are a hole, its left neighbour is far (t = 0, the background): every hole pixel shows source c - 1
    xs = [min(x + 4, c - 1) if x < c + 4 else x - 4 for x in range(w)]
    out = sr.view(img, depth, n, 8.0, 0.5)
    assert np.array_equal(out, from_columns(img, xs))
    assert np.array_equal(out[:, c - 4:c + 4], np.repeat(img[:, c - 1:c], 8, axis=1))
    # shift -8: far moves by +4, near by -4 -- they overlap on [c - 4, c + 3], where near (the larger t) covers far; the 4
    # targets vacated at either edge have one neighbour each
    xs = [0 if x < 4 else (x - 4 if x < c - 4 else min(x + 4, w - 1)) for x in range(w)]
    out = sr.view(img, depth, n, -8.0, 0.5)
    assert np.array_equal(out, from_columns(img, xs))
    assert np.array_equal(out[:, c - 4:c + 4], img[:, c:c + 8])
    # the same scene with the near plateau on the left: the hole is filled from its right neighbour, the far plateau
    out = sr.view(img, depth[:, ::-1], n, -8.0, 0.5)
    c2 = w - c                                      # far from c2 on; near [0, c2) moves by -4, far by +4
    assert np.array_equal(out[:, c2 - 4:c2 + 4], np.repeat(img[:, c2:c2 + 1], 8, axis=1))


def test_equal_background_on_both_sides_of_a_hole_takes_the_left_one():
    n, w = 3, 30                                    # a far column range in a near plane, pivot at near: far moves, near stays
    img = image((2, w))
    depth = np.full((2, w), n - 1, np.float32)
    depth[:, 10:14] = 0
    # shift 6, pivot 1: near d = 0, far d = -6: far lands on [4, 7], where near (larger t) already is -- far is hidden.
    # Targets 10 .. 13 are a hole between two near targets of equal t: the left one, source 9
    out = sr.view(img, depth, n, 6.0, 1.0)
    xs = [9 if 10 <= x < 14 else x for x in range(w)]
    assert np.array_equal(out, from_columns(img, xs))


def test_no_source_at_all_keeps_the_pixel():
    """N == 1: t = 0 everywhere; with pivot 1 and a shift as wide as allowed every source but few leaves the row"""
    w = 9
    img = image((2, w))
    out = sr.view(img, np.zeros((2, w), np.float32), 1, 8.0, 1.0)      # d = -8: only source 8 lands, on target 0
    assert np.array_equal(out, np.repeat(img[:, 8:9], w, axis=1))
    # a row whose single landing target is filled and every other target takes that one side
    assert np.array_equal(sr.source_columns(np.zeros(w, np.float32), 1, 8.0, 1.0, "last"), np.full(w, 8))


@pytest.mark.parametrize("n", [5, 9])
def test_near_first_mirrors_the_depth(n):
    """N - 1 a power of two and depths in quarters: z / (N - 1), 1 - z / (N - 1) and (N - 1) - z are all exact, so both forms
    give every source the same t"""
    rng = np.random.default_rng(n)
    img = image((5, 90), np.uint16)
    z = (rng.integers(0, 4 * (n - 1) + 1, (5, 90)) / 4.0).astype(np.float32)
    for shift in (13.0, -7.5):
        assert np.array_equal(sr.view(img, z, n, shift, 0.4, "first"), sr.view(img, np.float32(n - 1) - z, n, shift, 0.4, "last"))
    assert not np.array_equal(sr.view(img, z, n, 13.0, 0.4, "first"), sr.view(img, z, n, 13.0, 0.4, "last"))


def test_depth_outside_the_stack_is_clamped():
    n = 7
    rng = np.random.default_rng(3)
    img = image((4, 60))
    z = rng.integers(0, n, (4, 60)).astype(np.float32)
    over = z.copy()
    over[z == n - 1] += np.float32(1e-3)
    over[z == 0] -= np.float32(1e-3)
    assert (over > n - 1).any() and (over < 0).any()
    for near in ("last", "first"):
        assert np.array_equal(sr.view(img, over, n, 11.0, 0.5, near), sr.view(img, z, n, 11.0, 0.5, near))
    assert sr.nearness(np.float32([-0.5, 6.5, 3.0]), n).tolist() == [0.0, 1.0, 0.5]
    assert sr.nearness(np.float32([np.nan, np.inf, -np.inf, -0.0]), n).tobytes() == np.float32([0.0, 1.0, 0.0, 0.0]).tobytes()


def test_half_way_products_round_to_even():
    t = np.float32([0.0, 0.25, 0.5, 0.75, 1.0])
    assert sr.displacement(t, 2.0, 0.0).tolist() == [0, 0, 1, 2, 2]             # 0.5 -> 0, 1.5 -> 2
    assert sr.displacement(t, -7.5, 0.5 - 1.0 / 3.0).dtype == np.int32
    assert sr.displacement(np.float32([1.0]), 5.0, 0.5).tolist() == [2] and sr.displacement(np.float32([0.0]), 5.0, 0.5).tolist() == [-2]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_pair_layouts_and_anaglyph_channels(dtype):
    n, sep = 6, 14.0
    rng = np.random.default_rng(8)
    img = image((7, 50), dtype)
    z = (rng.random((7, 50)) * (n - 1)).astype(np.float32)
    left, right = sr.view(img, z, n, 7.0, 0.5), sr.view(img, z, n, -7.0, 0.5)
    assert not np.array_equal(left, right)
    par = sr.pair(img, z, n, sep, layout="parallel")
    assert par.shape == (7, 100, 3) and np.array_equal(par[:, :50], left) and np.array_equal(par[:, 50:], right)
    cross = sr.pair(img, z, n, sep, layout="cross")
    assert np.array_equal(cross[:, :50], right) and np.array_equal(cross[:, 50:], left)
    ana = sr.pair(img, z, n, sep, layout="anaglyph")
    assert ana.shape == img.shape and ana.dtype == img.dtype
    assert np.array_equal(ana[:, :, 2], left[:, :, 2]) and np.array_equal(ana[:, :, :2], right[:, :, :2])
    # the module's own host composition is the same routing
    for layout, want in (("parallel", par), ("cross", cross), ("anaglyph", ana)):
        assert np.array_equal(stereo.compose(left, right, layout), want)
    with pytest.raises(InvalidOptionError):
        stereo.compose(left, right[:, :40], "parallel")


def test_rocking_shifts():
    for sep, views in ((32.0, 9), (10.0, 2), (7.0, 4), (128.0, 11), (0.3, 7)):
        got = stereo.rocking_shifts(sep, views)
        want = [float(np.float32(-sep / 2.0 + k * sep / (views - 1))) for k in range(views)]
        assert got == want == [float(s) for s in sr.rocking_shifts(sep, views)]
        assert len(got) == views and got[0] == float(np.float32(-sep / 2)) and got[-1] == float(np.float32(sep / 2)) and all(a < b for a, b in zip(got, got[1:]))
        assert all(float(np.float32(s)) == s and abs(s) <= stereo.MAX_SHIFT for s in got)
    assert stereo.rocking_shifts(32.0, 9)[4] == 0.0
    assert stereo.rocking_shifts(7.0, 4)[1] == float(np.float32(-3.5 + 7.0 / 3))       # one rounding, from float64


# ------------------------------------------------------------------ host logic of the module
def test_option_checks():
    assert stereo.check_shift(64) == 64.0 and stereo.check_shift(-64.0, 65) == -64.0 and stereo.check_shift(0.1) == float(np.float32(0.1))
    for bad in (64.5, -65, float("nan"), float("inf"), "3", None, True):
        with pytest.raises(InvalidOptionError):
            stereo.check_shift(bad)
    with pytest.raises(InvalidOptionError):
        stereo.check_shift(7.5, 8)                  # ceil(|shift|) < W
    assert stereo.check_shift(7.0, 8) == 7.0
    assert stereo.check_separation(128) == 128.0 and stereo.check_separation(0.5, 2) == 0.5
    for bad in (0, -4.0, 128.5, float("nan"), "8", None):
        with pytest.raises(InvalidOptionError):
            stereo.check_separation(bad)
    with pytest.raises(InvalidOptionError):
        stereo.check_separation(20.0, 10)
    for bad in (-0.01, 1.01, float("nan"), "0.5", None):
        with pytest.raises(InvalidOptionError):
            stereo.check_pivot(bad)
    assert stereo.check_pivot(0) == 0.0 and stereo.check_pivot(1) == 1.0
    for bad in ("middle", None, 0):
        with pytest.raises(InvalidOptionError):
            stereo.check_near(bad)
    for bad in ("sidebyside", None, 2):
        with pytest.raises(InvalidOptionError):
            stereo.check_layout(bad)
    for bad in (1, 0, 2.0, "9", None, True):
        with pytest.raises(InvalidOptionError):
            stereo.check_views(bad)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(InvalidOptionError):
            stereo.check_n_frames(bad)
    with pytest.raises(InvalidOptionError):
        stereo.rocking_shifts(200.0, 9)
    with pytest.raises(InvalidOptionError):
        stereo.rocking_shifts(20.0, 1)


def test_entry_points_refuse_bad_arguments_before_they_look_for_a_device():
    from shinestacker_amd import BitDepthError
    img, z = image((8, 20)), np.zeros((8, 20), np.float32)
    bad_calls = [
        lambda: stereo.view(img, z, 4, 65.0), lambda: stereo.view(img, z, 4, 20.0), lambda: stereo.view(img, z, 0, 2.0),
        lambda: stereo.view(img, z, 4, 2.0, pivot=1.5), lambda: stereo.view(img, z, 4, 2.0, near="front"),
        lambda: stereo.view(img, z[:7], 4, 2.0), lambda: stereo.view(img[:, :, :2], z, 4, 2.0), lambda: stereo.view(img[0], z[0], 4, 2.0),
        lambda: stereo.pair(img, z, 4, 0.0), lambda: stereo.pair(img, z, 4, 130.0), lambda: stereo.pair(img, z, 4, 40.0),
        lambda: stereo.pair(img, z, 4, layout="wiggle"), lambda: stereo.pair(img, z, 4, 8.0, pivot=-1),
        lambda: stereo.rocking(img, z, 4, 8.0, views=1), lambda: stereo.rocking(img, z, 4, 8.0, near=None),
        lambda: stereo.view_device(1, 2, 3, 8, 20, np.uint8, 4, 99.0), lambda: stereo.view_device(1, 2, 3, 0, 20, np.uint8, 4, 1.0),
        lambda: stereo.pair_device(1, 2, 8, 20, np.uint8, 4, 0.0), lambda: stereo.pair_device(1, 2, 8, 20, np.uint8, 4, 8.0, layout="x"),
    ]
    for call in bad_calls:
        with pytest.raises(InvalidOptionError):
            call()
    for call in (lambda: stereo.view(img.astype(np.float32), z, 4, 2.0), lambda: stereo.pair(img.astype(np.int16), z, 4),
                 lambda: stereo.view_device(1, 2, 3, 8, 20, np.float32, 4, 1.0)):
        with pytest.raises(BitDepthError):
            call()


def test_without_a_gpu_the_calls_fail_loudly(hiplib):
    """no CPU path: DeviceError where no device is visible (where one is, the same calls give the restatement's result)"""
    img = image((6, 40))
    z = (np.random.default_rng(4).random((6, 40)) * 3).astype(np.float32)
    calls = (lambda: stereo.view(img, z, 4, 5.0), lambda: stereo.pair(img, z, 4, 10.0, layout="anaglyph"),
             lambda: stereo.rocking(img, z, 4, 10.0, views=3)[2])
    wants = (lambda: sr.view(img, z, 4, 5.0), lambda: sr.pair(img, z, 4, 10.0, layout="anaglyph"),
             lambda: sr.rocking(img, z, 4, 10.0, views=3)[2])
    for call, want in zip(calls, wants):
        if hiplib.device_count() < 1:
            with pytest.raises(DeviceError):
                call()
        else:
            assert np.array_equal(call(), want())


def test_c_entry_points_validate_without_a_gpu(hiplib):
    lib = hiplib.load()
    img, z, out = image((8, 20)), np.zeros((8, 20), np.float32), np.empty((8, 20, 3), np.uint8)
    p, d, o = img.ctypes.data, z.ctypes.data, out.ctypes.data
    U8, INV = hiplib.MI_U8, hiplib.MI_ERR_INVALID

    def both(img_p, depth_p, out_p, h, w, dtype, n, shift, pivot, near_first):
        return (lib.mi_stereo_view(0, img_p, depth_p, out_p, h, w, dtype, n, shift, pivot, near_first),
                lib.mi_stereo_view_device(0, None, img_p, depth_p, out_p, h, w, dtype, n, shift, pivot, near_first))
    for args in ((None, d, o, 8, 20, U8, 4, 2.0, 0.5, 0), (p, None, o, 8, 20, U8, 4, 2.0, 0.5, 0), (p, d, None, 8, 20, U8, 4, 2.0, 0.5, 0),
                 (p, d, o, 8, 20, hiplib.MI_F32, 4, 2.0, 0.5, 0), (p, d, o, 8, 20, 99, 4, 2.0, 0.5, 0),
                 (p, d, o, 0, 20, U8, 4, 2.0, 0.5, 0), (p, d, o, 8, 0, U8, 4, 2.0, 0.5, 0), (p, d, o, 8, 20, U8, 0, 2.0, 0.5, 0),
                 (p, d, o, 8, 20, U8, 4, 64.5, 0.5, 0), (p, d, o, 8, 20, U8, 4, -65.0, 0.5, 0), (p, d, o, 8, 20, U8, 4, float("nan"), 0.5, 0),
                 (p, d, o, 8, 20, U8, 4, float("inf"), 0.5, 0), (p, d, o, 8, 20, U8, 4, 19.5, 0.5, 0), (p, d, o, 8, 20, U8, 4, -20.0, 0.5, 0),
                 (p, d, o, 8, 20, U8, 4, 2.0, -0.1, 0), (p, d, o, 8, 20, U8, 4, 2.0, 1.1, 0), (p, d, o, 8, 20, U8, 4, 2.0, float("nan"), 0),
                 (p, d, o, 8, 20, U8, 4, 2.0, 0.5, 2)):
        assert both(*args) == (INV, INV), args
        assert lib.mi_last_error()
    # the device form gathers from the whole row: the view needs a buffer of its own
    assert lib.mi_stereo_view_device(0, None, p, d, p, 8, 20, U8, 4, 2.0, 0.5, 0) == INV
    for args in ((None, p, o, 8, 20, U8, 2), (p, None, o, 8, 20, U8, 2), (p, o, None, 8, 20, U8, 2), (p, o, o, 8, 20, U8, 0),
                 (p, o, p, 8, 20, U8, 0), (p, p + 4, o, 8, 20, hiplib.MI_F32, 2), (p, p + 4, o, 0, 20, U8, 2), (p, p + 4, o, 8, 20, U8, 3),
                 (p, p + 4, o, 8, 20, U8, -1), (p, p + 1, o, 8, 20, U8, 2)):
        assert lib.mi_stereo_compose_device(0, None, *args) == INV, args
    assert stereo.LAYOUTS == {"parallel": 0, "cross": 1, "anaglyph": 2}
    text = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "mi355stack.h")).read()
    for name, code in (("PARALLEL", 0), ("CROSS", 1), ("ANAGLYPH", 2)):
        assert f"MI_STEREO_{name} = {code}" in text


# ------------------------------------------------------------------ actions and pipeline, as far as no device is needed
class _NoDepthMapStacker:
    process = None
    do_step_callback = False

    def name(self):
        return "plain"

    def steps_per_frame(self):
        return 1


def test_actions_take_the_stereo_options_and_reject_a_stacker_without_a_depth_map():
    from shinestacker_amd import FocusStack, FocusStackBunch, PyramidStack
    for action in (FocusStack, FocusStackBunch):
        with pytest.raises(InvalidOptionError) as e:
            action("stack", _NoDepthMapStacker(), stereo_path="stereo")
        assert "depth map" in str(e.value)
        a = action("stack", _NoDepthMapStacker())                       # off: the stacker is not asked for anything
        assert a.stereo_path is None
        a = action("stack", PyramidStack(), stereo_path="stereo")
        assert (a.stereo_layout, a.stereo_separation, a.stereo_pivot, a.stereo_near) == ("anaglyph", stereo.DEFAULT_SEPARATION, 0.5, "last")
        a = action("stack", PyramidStack(), stereo_path="3d", stereo_layout="cross", stereo_separation=20, stereo_pivot=0.25,
                   stereo_near="first", depth_map_sigma=1.0)
        assert (a.stereo_path, a.stereo_layout, a.stereo_separation, a.stereo_pivot, a.stereo_near) == ("3d", "cross", 20, 0.25, "first")
        for bad in (dict(stereo_layout="wiggle"), dict(stereo_separation=0), dict(stereo_separation=129.0), dict(stereo_pivot=2),
                    dict(stereo_near="front"), dict(depth_map_sigma=17.0)):
            with pytest.raises(InvalidOptionError):
                action("stack", PyramidStack(), stereo_path="stereo", **bad)


def test_pipeline_checks_the_stereo_option_before_anything_else():
    from shinestacker_amd import pipeline
    for fn in (pipeline.align_and_stack, pipeline.align_and_stack_device):
        par = inspect.signature(fn).parameters
        assert par["stereo"].default is None and par["stereo"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    frames = [np.zeros((40, 60, 3), np.uint8)] * 2
    for bad, info in ((dict(layout="wiggle"), {}), (dict(separation=0), {}), (dict(pivot=3), {}), (dict(near="x"), {}),
                      (dict(sigma=99.0), {}), (dict(colour="red"), {}), (dict(separation=128.0), {}), (7, {}), (dict(), None)):
        with pytest.raises(InvalidOptionError):
            pipeline.align_and_stack(frames, stereo=bad, info=info)
        with pytest.raises(InvalidOptionError):
            pipeline.align_and_stack_device(1, 2, 40, 60, np.uint8, stereo=bad, info=info)
    opts = pipeline._check_stereo({"separation": 10}, {}, (40, 60), None)
    assert opts == {"layout": "anaglyph", "separation": 10, "pivot": 0.5, "near": "last", "sigma": 2.0}
    assert pipeline._check_stereo({"sigma": 0}, {}, (40, 60), 3.0)["sigma"] == 0.0
    assert pipeline._check_stereo({}, {}, (40, 60), 3.0)["sigma"] == 3.0


def test_package_exports_the_module():
    import shinestacker_amd as sa
    assert sa.stereo is stereo and "stereo" in sa.__all__
    for name in ("view", "view_device", "pair", "pair_device", "rocking", "rocking_shifts", "compose"):
        assert callable(getattr(stereo, name))
    par = inspect.signature(stereo.pair).parameters
    assert (par["separation"].default, par["pivot"].default, par["near"].default, par["layout"].default) == \
        (stereo.DEFAULT_SEPARATION, 0.5, "last", "parallel")
    assert inspect.signature(stereo.rocking).parameters["views"].default == 9
    assert stereo.MAX_SHIFT == sr.MAX_SHIFT == 64.0 and 0 < stereo.DEFAULT_SEPARATION <= stereo.MAX_SEPARATION == 128.0
