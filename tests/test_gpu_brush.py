"""GPU: brush retouching -- the stroke kernel and the blend kernel (csrc/kernels_brush.hpp) behind retouch.stroke / stroke_device /
apply / blend, the pipeline's and the action's retouch= -- every comparison is array_equal against tests/golden/brush.{npz,json}
(recorded from the reference's own brush code, tools/gen_golden_brush.py) or against the NumPy restatement's fold."""
import json
import os
import shutil

import numpy as np
import pytest

import brush_restatement as br
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(hiplib):
    hiplib.require_device()
    with open(os.path.join(GOLDEN, "brush.json")) as fh:
        return json.load(fh), load_golden("brush")


@pytest.fixture(scope="module")
def rt(hiplib):
    hiplib.require_device()
    from shinestacker_amd import retouch
    return retouch


def frames(shape, dtype, seed=0):
    rng = np.random.default_rng(100 + seed)
    hi = np.iinfo(dtype).max + 1
    return rng.integers(0, hi, shape + (3,)).astype(dtype), rng.integers(0, hi, shape + (3,)).astype(dtype)


def want(rt, master, source, points, size, hardness=50, opacity=100, flow=100):
    """the restatement's fold with the table brush_mask gives (held to the recorded tables by the CPU tests)"""
    r = br.radius_of(size)
    return br.stroke_fold(master, source, rt.brush_mask(2 * r + 1, hardness, opacity), br.centres(points), r, opacity, flow)


def check(rt, master, source, points, size, hardness=50, opacity=100, flow=100):
    keep_m, keep_s = master.copy(), source.copy()
    out, area, layer = rt.stroke(master, source, points, size, hardness, opacity, flow, return_mask=True)
    w_out, w_layer, w_area = want(rt, master, source, points, size, hardness, opacity, flow)
    assert out.dtype == master.dtype and out.shape == master.shape and layer.dtype == np.float64
    assert np.array_equal(layer, w_layer), int((layer != w_layer).sum())
    assert np.array_equal(out, w_out), int((out != w_out).sum())
    assert tuple(area) == tuple(w_area)
    assert np.array_equal(master, keep_m) and np.array_equal(source, keep_s)
    return out, layer


def test_every_recorded_stroke(gold, rt):
    """the reference's own frames, mask layers and undo areas: five brushes on both depths over 34 stamps that include clipped
    ones at every edge and ones outside the frame, strokes that miss the frame or are empty, a single stamp, a flow-7 run"""
    meta, z = gold
    for c in meta["cases"]:
        size, hardness, opacity, flow = c["brush"]
        master, source = z["master_" + c["frame"]], z["source_" + c["frame"]]
        out, area, layer = rt.stroke(master, source, meta["stamp_lists"][c["points"]], size, hardness, opacity, flow, return_mask=True)
        assert np.array_equal(layer, z[c["layer"]]), c["name"]
        assert out.dtype == master.dtype and np.array_equal(out, z[c["out"]]), c["name"]
        assert list(area) == c["area"], c["name"]
        plain, area2 = rt.stroke(master, source, meta["stamp_lists"][c["points"]], size, hardness, opacity, flow)
        assert np.array_equal(plain, out) and area2 == area


def scribble(h, w, n, seed):
    """n positions: a walk across the frame with half-way coordinates, some a little outside every edge"""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-3, w + 2, n) + rng.integers(-2, 3, n) * 0.5
    ys = (h / 2) * (1 + np.sin(np.linspace(0, 5, n))) + rng.integers(-4, 5, n) * 0.5 - 1
    return list(zip(xs.tolist(), ys.tolist()))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", [(5, 7), (37, 53), (131, 197), (40, 600)])
def test_frame_shapes_radii_and_hardness(rt, shape, dtype):
    """(5, 7): smaller than a tile, radius 2 only fits twice; (131, 197): odd rows put 3- and 6-byte pixels on every alignment,
    9 x 4 tiles; (40, 600): 10 tiles in a row.  Radius 2 and 15; hardness 0, 50 and 100."""
    master, source = frames(shape, dtype)
    h, w = shape
    pts = scribble(h, w, 24 if w < 100 else 60, 1)
    for size, hardness, opacity, flow in ((5, 50, 100, 100), (5, 0, 80, 60), (31, 0, 100, 40), (31, 50, 90, 100), (31, 100, 100, 100),
                                          (5, 100, 35, 100)):
        out, _ = check(rt, master, source, pts, size, hardness, opacity, flow)
        assert not np.array_equal(out, master)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_a_brush_larger_than_the_frame(rt, dtype):
    master, source = frames((37, 53), dtype, 1)
    out, layer = check(rt, master, source, [(26, 18), (0, 0), (60, 40), (-50, 18)], 121, 50, 100, 30)     # radius 60
    assert (layer > 0).mean() > 0.9


def test_fold_order_over_more_than_one_chunk(rt):
    """600 stamps at flow 7 whose squares all hold one tile: more than one LDS chunk of 512, and sums of 600 different doubles
    that depend on the order they are added in -- shuffled, the restatement itself gives another mask layer."""
    master, source = frames((16, 64), np.uint16, 2)
    rng = np.random.default_rng(5)
    pts = [(float(x), float(y)) for x, y in zip(rng.integers(20, 44, 600) + rng.integers(0, 2, 600) * 0.5, rng.integers(0, 16, 600))]
    size, hardness, opacity, flow = 131, 20, 0.9, 7                                           # radius 65 >= the tile's extent
    out, layer = check(rt, master, source, pts, size, hardness, opacity, flow)
    assert 0 < layer.min() and layer.max() < 1
    shuffled = [pts[i] for i in rng.permutation(600)]
    assert not np.array_equal(want(rt, master, source, shuffled, size, hardness, opacity, flow)[1], layer)
    # with the clip inside the fold the order matters again once the mask saturates
    pts = [(30.0 + (k % 7), 8.0) for k in range(600)]
    out, layer = check(rt, master, source, pts, 131, 20, 100, 7)
    assert layer.max() == 1.0


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_flow_100_repeated_saturates_the_mask(rt, dtype):
    master, source = frames((37, 53), dtype, 3)
    out, layer = check(rt, master, source, [(20, 18)] * 5 + [(21.5, 18.5)] * 4, 31, 50, 100, 100)
    assert (layer == 1.0).sum() > 50
    sat = layer == 1.0
    assert np.array_equal(out[sat], source[sat])                                                  # e = 1: the source itself
    out, layer = check(rt, master, source, [(20, 18)] * 9, 31, 100, 60, 100)                     # opacity twice: M saturates, e = 0.6
    assert layer.max() == 1.0


def test_an_l_shaped_stroke_leaves_the_tiles_it_does_not_meet(rt):
    """the bounding box of the L holds tiles no stamp meets: they equal the master, and so does everything outside the squares"""
    master, source = frames((160, 330), np.uint8, 4)
    pts = [(10.0, 8.0 + 6 * k) for k in range(24)] + [(10.0 + 8 * k, 146.0) for k in range(38)]
    out, layer = check(rt, master, source, pts, 13, 50, 100, 100)
    assert np.array_equal(out[:128, 64:], master[:128, 64:]) and not layer[:128, 64:].any()
    assert not np.array_equal(out[:, :17], master[:, :17]) and not np.array_equal(out[140:153], master[140:153])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_clipped_outside_and_empty_strokes(rt, dtype):
    h, w = 37, 53
    master, source = frames((h, w), dtype, 5)
    edges = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w / 2, -3), (w / 2, h + 2), (-4, h / 2), (w + 3, h / 2)]
    out, layer = check(rt, master, source, edges, 11, 50, 100, 100)
    assert layer[0, 0] > 0 and layer[h - 1, w - 1] > 0 and layer[0, w - 1] > 0 and layer[h - 1, 0] > 0
    outside = [(-6, 10), (w + 5, 10), (10, -6), (10, h + 5), (-1e6, -1e6)]
    out, area, layer = rt.stroke(master, source, outside + [(-1e9, -1e9), (1e12, 5), (5, -1e300)], 11, return_mask=True)
    assert np.array_equal(out, master) and area == (0, 0, 0, 0) and not layer.any()
    out, area, layer = rt.stroke(master, source, [], 11, return_mask=True)
    assert np.array_equal(out, master) and area == (0, 0, 0, 0) and not layer.any() and layer.shape == (h, w)
    check(rt, master, source, outside + [(5, 5)] + outside, 11)                                  # one hit among the misses


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_blend_from_a_mask(rt, dtype):
    master, source = frames((37, 53), dtype, 6)
    rng = np.random.default_rng(7)
    for mask, opacity in ((np.zeros((37, 53)), 100), (np.ones((37, 53)), 100), (np.ones((37, 53)), 55), (np.full((37, 53), 2.5), 100),
                          (np.full((37, 53), 2.5), 30), (rng.random((37, 53)), 100), (rng.random((37, 53)) * 3 - 1, 70),
                          (rng.random((37, 53)).astype(np.float32), 100)):
        out = rt.blend(master, source, mask, opacity)
        assert out.dtype == master.dtype and np.array_equal(out, br.blend(master, source, mask, opacity))
    assert np.array_equal(rt.blend(master, source, np.zeros((37, 53))), master)
    assert np.array_equal(rt.blend(master, source, np.ones((37, 53))), source)
    assert np.array_equal(rt.blend(master, source, np.full((37, 53), 7.0)), source)


def test_apply_runs_the_strokes_in_order_from_two_sources(rt):
    from shinestacker_amd import Stroke
    master, a = frames((60, 90), np.uint16, 8)
    b, _ = frames((60, 90), np.uint16, 9)
    strokes = [Stroke(0, rt.stamps_along([(5, 5), (80, 50)], 21), 21, 50, 100, 60),
               Stroke(1, rt.stamps_along([(80, 5), (5, 50)], 31), 31, 0, 80, 100),       # crosses the first
               Stroke(0, [(45, 28), (46, 28), (-30, -30)], 9, 100, 100, 100)]
    got = rt.apply(master, strokes, {0: a, 1: b})
    wanted = master
    for s in strokes:
        wanted = want(rt, wanted, (a, b)[s.source], s.points, *s.brush())[0]
    assert np.array_equal(got, wanted) and not np.array_equal(got, master)
    assert np.array_equal(rt.apply(master, strokes, [a, b]), wanted)                              # a sequence indexed by the source
    assert np.array_equal(rt.apply(master, [], {}), master)
    swapped = rt.apply(master, strokes[::-1], {0: a, 1: b})
    assert not np.array_equal(swapped, wanted)


def test_stroke_device_paints_in_place_and_only_reads_the_source(hiplib, rt):
    master, source = frames((70, 130), np.uint8, 10)
    pts = rt.stamps_along([(-5, 10), (120, 60)], 25)
    m, s, k = hiplib.DeviceBuffer(master.nbytes), hiplib.DeviceBuffer(source.nbytes), hiplib.DeviceBuffer(70 * 130 * 8)
    try:
        m.upload(master)
        s.upload(source)
        k.upload(np.full((70, 130), 9.0))                                                         # the call zeroes the plane first
        area = rt.stroke_device(m.ptr, s.ptr, 70, 130, np.uint8, pts, 25, 50, 100, 50, dev_mask=k.ptr)
        w_out, w_layer, w_area = want(rt, master, source, pts, 25, 50, 100, 50)
        assert np.array_equal(m.download(master.shape, np.uint8), w_out) and tuple(area) == tuple(w_area)
        assert np.array_equal(k.download((70, 130), np.float64), w_layer)
        assert np.array_equal(s.download(source.shape, np.uint8), source)
        # a second stroke paints on the first one's result
        area = rt.stroke_device(m.ptr, s.ptr, 70, 130, np.uint8, [(60, 30)], 41, 0, 100, 100)
        assert np.array_equal(m.download(master.shape, np.uint8), want(rt, w_out, source, [(60, 30)], 41, 0, 100, 100)[0])
        assert area == (40, 10, 81, 51)
        with pytest.raises(ValueError):
            rt.stroke_device(m.ptr, m.ptr, 70, 130, np.uint8, pts, 25)
        # blend_device, in place too
        k.upload(w_layer)
        m.upload(master)
        rt.blend_device(m.ptr, s.ptr, k.ptr, 70, 130, np.uint8, 100)
        hiplib.check(hiplib.load().mi_device_synchronize(0))
        assert np.array_equal(m.download(master.shape, np.uint8), br.blend(master, source, w_layer, 100))
    finally:
        for b in (m, s, k):
            b.free()


def test_pipeline_paints_from_the_frames_as_they_were_pushed(hiplib, rt):
    """align_and_stack(retouch=...) == the strokes restated on the result of the same call without them, the source being the
    reference frame itself, respectively the moving frame through the library's own warp with the matrix the estimator gave;
    the filters come after the strokes"""
    from shinestacker_amd import Stroke, denoise, unsharp_mask
    from shinestacker_amd.align import _BORDER_CODE, _DEFAULT_ALIGNMENT_CONFIG
    from shinestacker_amd.imageio import read_img
    from shinestacker_amd.pipeline import align_and_stack
    names = sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop")))
    fr = [read_img(os.path.join(GOLDEN, "img_jpg_crop", n)) for n in names]
    h, w = fr[0].shape[:2]
    ref_idx, moving = len(fr) // 2, 1
    mats = [np.array([[1.0, 0.0, 0.75 * (i + 1)], [0.0, 1.0, -0.5 * i - 0.25]]) for i in range(len(fr))]

    def est(i0, i1, fc, mc, ac):
        i = next(k for k, f in enumerate(fr) if np.array_equal(f, i0))
        assert np.array_equal(i1, fr[ref_idx])
        return 500, mats[i]
    kw = dict(estimator=est, alignment_config={'subsample': 1})
    strokes = [Stroke(ref_idx, rt.stamps_along([(10, 10), (w - 10, h // 2)], 41), 41, 50, 100, 80),
               Stroke(moving, rt.stamps_along([(w // 2, -5), (w // 3, h + 5)], 25), 25, 0, 100, 100)]
    plain, _ = align_and_stack(fr, **kw)
    got, _ = align_and_stack(fr, retouch=strokes, **kw)
    cfg = _DEFAULT_ALIGNMENT_CONFIG
    warped = hiplib.warp_affine(fr[moving], mats[moving], _BORDER_CODE[cfg['border_mode']], cfg['border_value'], 21, cfg['border_blur'])
    assert not np.array_equal(warped, fr[moving])
    wanted = want(rt, plain, fr[ref_idx], strokes[0].points, *strokes[0].brush())[0]
    wanted = want(rt, wanted, warped, strokes[1].points, *strokes[1].brush())[0]
    assert np.array_equal(got, wanted) and not np.array_equal(got, plain)
    assert np.array_equal(align_and_stack(fr, retouch=None, **kw)[0], plain) and np.array_equal(align_and_stack(fr, retouch=[], **kw)[0], plain)
    full, _ = align_and_stack(fr, retouch=strokes, denoise_amount=3, unsharp=(1.0, 0.5, 0), **kw)
    assert np.array_equal(full, unsharp_mask(denoise(wanted, 3, 3), 1.0, 0.5, 0))


def test_focus_stack_action_paints_before_it_writes(hiplib, rt, tmp_path):
    from shinestacker_amd import FocusStack, PyramidStack, StackJob, Stroke
    from shinestacker_amd.imageio import read_img
    src = os.path.join(GOLDEN, "img_jpg_crop")
    names = sorted(os.listdir(src))
    os.makedirs(tmp_path / "input")
    for n in names:
        shutil.copy(os.path.join(src, n), tmp_path / "input" / n)
    fr = [read_img(os.path.join(src, n)) for n in names]
    h, w = fr[0].shape[:2]
    strokes = [Stroke(1, rt.stamps_along([(5, 5), (w - 5, h - 5)], 31), 31, 50, 100, 100),
               Stroke(names[4], [(w // 2, h // 2)] * 3, 61, 20, 70, 50), Stroke(1, [(w, 0)], 15)]
    outs = {}
    for key, opt in (("plain", None), ("painted", strokes)):
        job = StackJob("job", str(tmp_path), input_path="input")
        job.add_action(FocusStack("stack", PyramidStack(), output_path="out-" + key, prefix="p_", retouch=opt))
        job.run()
        outs[key] = read_img(os.path.join(str(tmp_path), "out-" + key, "p_" + names[0]))
    wanted = outs["plain"]
    for s, frame in zip(strokes, (fr[1], fr[4], fr[1])):
        wanted = want(rt, wanted, frame, s.points, *s.brush())[0]
    assert np.array_equal(outs["painted"], wanted) and not np.array_equal(wanted, outs["plain"])
