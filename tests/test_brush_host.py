"""CPU: brush retouching as far as no device is needed -- the stamp table and the NumPy restatement against frames recorded
from the reference's own brush code (tests/golden/brush.*, tools/gen_golden_brush.py), the viewer's stamp interpolation on
hand-checked polylines, the option and argument checks, and the action's trace with the option off."""
import inspect
import json
import os
import shutil

import numpy as np
import pytest

import brush_restatement as br
from conftest import GOLDEN, load_golden
from shinestacker_amd import BitDepthError, DeviceError, InvalidOptionError, ShapeError, Stroke, retouch


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "brush.json")) as fh:
        meta = json.load(fh)
    return meta, load_golden("brush")


def case_inputs(meta, z, c):
    size, hardness, opacity, flow = c["brush"]
    return (z["master_" + c["frame"]], z["source_" + c["frame"]], meta["stamp_lists"][c["points"]], size, hardness, opacity, flow)


def test_fixture_holds_the_cases_the_issue_names(gold):
    meta, z = gold
    assert meta["brushes"] == [[5, 50, 100, 100], [13, 0, 70, 30], [21, 100, 100, 50], [9.7, 85, 55, 100], [30, 20, 100, 7]]
    assert len(meta["cases"]) >= 12 and len(meta["stamp_lists"]["edges"]) == 34
    for c in meta["cases"]:
        assert z["master_" + c["frame"]].shape[0] <= 48 and z["master_" + c["frame"]].shape[1] <= 64
    h, w = z["master_odd_uint8"].shape[:2]
    centres = br.centres(meta["stamp_lists"]["edges"])
    fps = [br.footprint(cx, cy, 2, h, w) for cx, cy in centres]
    assert sum(f is None for f in fps) >= 4                                                       # stamps that miss the frame
    hit = [f for f in fps if f is not None]
    assert any(f[0] == 0 for f in hit) and any(f[1] == 0 for f in hit) and any(f[2] == w for f in hit) and any(f[3] == h for f in hit)
    size = os.path.getsize(os.path.join(GOLDEN, "brush.npz")) + os.path.getsize(os.path.join(GOLDEN, "brush.json"))
    assert size < 200 * 1024


def test_brush_mask_equals_every_recorded_table(gold):
    meta, z = gold
    seen = set()
    for c in meta["cases"]:
        size, hardness, opacity, _ = c["brush"]
        r = retouch.brush_radius(size)
        assert r == br.radius_of(size)
        t = retouch.brush_mask(2 * r + 1, hardness, opacity)
        assert t.dtype == np.float64 and np.array_equal(t, z[c["table"]]), c["name"]
        seen.add(c["table"])
    assert len(seen) == 5


def test_brush_mask_profiles():
    """hardness 100 is a disc, the centre of an odd table is the opacity, nothing exceeds it and the corners are 0"""
    t = retouch.brush_mask(21, 100, 100)
    assert set(np.unique(t)) == {0.0, 1.0} and t[10, 10] == 1.0 and t[0, 0] == 0.0 and t[10, 0] == 1.0
    for hardness in (0, 20, 50, 85):
        t = retouch.brush_mask(31, hardness, 70)
        assert t[15, 15] == 0.7 and t.max() == 0.7 and t.min() == 0.0 and t[0, 0] == 0.0
        assert np.array_equal(t, t.T) and np.array_equal(t, t[::-1])
        assert np.all(np.diff(t[15, 15:]) <= 0)


@pytest.mark.parametrize("form", ["stroke_loop", "stroke_fold"])
def test_restatement_equals_every_recorded_stroke(gold, form):
    meta, z = gold
    for c in meta["cases"]:
        master, source, points, size, hardness, opacity, flow = case_inputs(meta, z, c)
        keep = master.copy()
        out, layer, area = getattr(br, form)(master, source, z[c["table"]], br.centres(points), br.radius_of(size), opacity, flow)
        assert np.array_equal(out, z[c["out"]]), c["name"]
        assert layer.dtype == np.float64 and np.array_equal(layer, z[c["layer"]]), c["name"]
        assert list(area) == c["area"], c["name"]
        assert np.array_equal(master, keep)


def test_area_and_centres_equal_the_recording(gold):
    meta, z = gold
    for c in meta["cases"]:
        master, _, points, size, *_ = case_inputs(meta, z, c)
        centres = retouch.stamp_centres(points)
        assert centres.dtype == np.int32 and [tuple(v) for v in centres.tolist()] == br.centres(np.clip(points, -2 ** 30, 2 ** 30))
        r = retouch.brush_radius(size)
        area = retouch.stroke_area(centres, r, *master.shape[:2])
        assert list(area) == c["area"], c["name"]
        box = retouch.stroke_box(centres, r, *master.shape[:2])
        assert area[0] <= box[0] and area[1] <= box[1] and area[2:] == box[2:]
    # half-way positions round to even, as Python's round does
    assert retouch.stamp_centres([(0.5, 1.5), (2.5, -0.5), (-1.5, 3.49)]).tolist() == [[0, 2], [2, 0], [-2, 3]]


def test_stamps_along_on_hand_checked_polylines():
    # a point: stamped once
    assert retouch.stamps_along([(3, 4)], 20) == [(3.0, 4.0)]
    assert retouch.stamps_along([], 20) == []
    # size 20: min_step 5.  A segment of length 4 is shorter: only the first point, and the anchor stays where it was ...
    assert retouch.stamps_along([(0, 0), (4, 0)], 20) == [(0.0, 0.0)]
    # ... so a further point is measured from (0, 0): distance 8 -> 1 step -> stamps at the anchor again and at the point
    assert retouch.stamps_along([(0, 0), (4, 0), (8, 0)], 20) == [(0.0, 0.0), (0.0, 0.0), (8.0, 0.0)]
    # a dog-leg: 12 along x (2 steps of 6), then 10 along y (2 steps of 5); every leg starts by stamping its anchor again
    assert retouch.stamps_along([(0, 0), (12, 0), (12, 10)], 20) == \
        [(0.0, 0.0), (0.0, 0.0), (6.0, 0.0), (12.0, 0.0), (12.0, 0.0), (12.0, 5.0), (12.0, 10.0)]
    # the zoom factor scales the step: at zoom 2 the 12-pixel leg is one step
    assert retouch.stamps_along([(0, 0), (12, 0)], 20, zoom=2.0) == [(0.0, 0.0), (0.0, 0.0), (12.0, 0.0)]
    # a diagonal: distance 5 with size 8 (min_step 2) -> 2 steps of (1.5, 2)
    assert retouch.stamps_along([(1, 1), (4, 5)], 8) == [(1.0, 1.0), (1.0, 1.0), (2.5, 3.0), (4.0, 5.0)]
    for bad in (lambda: retouch.stamps_along([(0, 0)], 0), lambda: retouch.stamps_along([(0, 0)], 10, zoom=0),
                lambda: retouch.stamps_along([(0, float("nan"))], 10), lambda: retouch.stamps_along([3], 10),
                lambda: retouch.stamps_along(7, 10)):
        with pytest.raises(InvalidOptionError):
            bad()


def frames(shape=(12, 16), dtype=np.uint8):
    rng = np.random.default_rng(3)
    hi = np.iinfo(dtype).max + 1
    return rng.integers(0, hi, shape + (3,)).astype(dtype), rng.integers(0, hi, shape + (3,)).astype(dtype)


def test_option_checks_come_before_the_device():
    m, s = frames()
    pts = [(5, 5)]
    bad = [lambda: retouch.stroke(m, s, pts, size=3), lambda: retouch.stroke(m, s, pts, size=1002), lambda: retouch.stroke(m, s, pts, size="big"),
           lambda: retouch.stroke(m, s, pts, hardness=101), lambda: retouch.stroke(m, s, pts, hardness=-1),
           lambda: retouch.stroke(m, s, pts, opacity=100.5), lambda: retouch.stroke(m, s, pts, flow=float("nan")),
           lambda: retouch.stroke(m, s, pts, flow=True), lambda: retouch.stroke(m, s, [(1, float("inf"))]),
           lambda: retouch.stroke(m, s, [(0, 0)] * (retouch.MAX_STAMPS + 1)), lambda: retouch.stroke(m[:, :, :2], s[:, :, :2], pts),
           lambda: retouch.stroke(m[0], s[0], pts),
           lambda: retouch.stroke_device(1, 2, 12, 16, np.uint8, pts, size=3), lambda: retouch.stroke_device(1, 2, 0, 16, np.uint8, pts),
           lambda: retouch.blend(m, s, np.zeros((12, 15))), lambda: retouch.blend(m, s, np.zeros((12, 16)), opacity=101),
           lambda: retouch.blend(m, s, np.full((12, 16), np.nan)), lambda: retouch.blend_device(1, 2, 3, 12, 16, np.uint8, opacity=-1),
           lambda: retouch.brush_mask(0, 50, 100), lambda: retouch.brush_mask(11, 150, 100), lambda: retouch.brush_mask(11.5, 50, 100),
           lambda: Stroke(0, pts, size=2), lambda: Stroke(1.5, pts), lambda: Stroke(None, pts), lambda: Stroke(0, [(1,)]),
           lambda: retouch.apply(m, [Stroke(3, pts)], {0: s}), lambda: retouch.apply(m, [Stroke(3, pts)], [s]),
           lambda: retouch.apply(m, [(0, pts)], {0: s}), lambda: retouch.apply(m, 5, {0: s}),
           lambda: retouch.apply_device(1, 12, 16, np.uint8, [Stroke("a", pts)], {0: 2})]
    for call in bad:
        with pytest.raises(InvalidOptionError):
            call()
    for call in (lambda: retouch.stroke(m.astype(np.float32), s.astype(np.float32), pts), lambda: retouch.stroke(m, s.astype(np.uint16), pts),
                 lambda: retouch.blend(m.astype(np.int16), s.astype(np.int16), np.zeros((12, 16))),
                 lambda: retouch.stroke_device(1, 2, 12, 16, np.float32, pts), lambda: retouch.blend_device(1, 2, 3, 12, 16, np.float64),
                 lambda: retouch.apply(m, [Stroke(0, pts)], {0: s.astype(np.uint16)})):
        with pytest.raises(BitDepthError):
            call()
    for call in (lambda: retouch.stroke(m, s[:, :15], pts), lambda: retouch.blend(m, s[:11], np.zeros((12, 16))),
                 lambda: retouch.apply(m, [Stroke(0, pts)], {0: s[:11]})):
        with pytest.raises(ShapeError):
            call()
    assert retouch.check_options() == 25 and retouch.check_options(5, 0, 0, 0) == 2 and retouch.check_options(1000) == 500
    assert retouch.brush_radius(9.7) == 4 and retouch.brush_radius(1001.9) == 500
    st = Stroke("0001.png", [(1, 2), (3.5, 4)], 13, 0, 70, 30)
    assert (st.source, st.points, st.radius, st.brush()) == ("0001.png", [(1.0, 2.0), (3.5, 4.0)], 6, (13, 0, 70, 30))
    par = inspect.signature(retouch.stroke).parameters
    assert [par[k].default for k in ("size", "hardness", "opacity", "flow", "device", "return_mask")] == [50, 50, 100, 100, 0, False]


def test_without_a_gpu_the_calls_fail_loudly(hiplib, gold):
    """no CPU path: DeviceError where no device is visible (where one is, the same calls give the recorded result)"""
    meta, z = gold
    c = meta["cases"][0]
    master, source, points, size, hardness, opacity, flow = case_inputs(meta, z, c)
    layer = z[c["layer"]]
    calls = (lambda: retouch.stroke(master, source, points, size, hardness, opacity, flow)[0],
             lambda: retouch.apply(master, [Stroke(0, points, size, hardness, opacity, flow)], [source]),
             lambda: retouch.blend(master, source, layer, opacity))
    for call in calls:
        if hiplib.device_count() < 1:
            with pytest.raises(DeviceError):
                call()
        else:
            assert np.array_equal(call(), z[c["out"]])


def test_c_entry_points_validate_without_a_gpu(hiplib):
    lib = hiplib.load()
    m, s = frames()
    table = np.zeros((5, 5))
    stamps = np.zeros((3, 2), np.int32)
    box = np.array([0, 0, 16, 12], np.int32)
    mp, sp, tp, cp, bp = (a.ctypes.data for a in (m, s, table, stamps, box))
    U8, INV = hiplib.MI_U8, hiplib.MI_ERR_INVALID

    def both(master, source, h, w, dtype, tab, radius, st, n, opacity):
        return (lib.mi_brush_stroke(0, master, source, h, w, dtype, tab, radius, st, n, opacity, None, None),
                lib.mi_brush_stroke_device(0, None, master, source, h, w, dtype, tab, radius, st, n, bp, opacity, None))
    for args in ((None, sp, 12, 16, U8, tp, 2, cp, 3, 1.0), (mp, None, 12, 16, U8, tp, 2, cp, 3, 1.0), (mp, mp, 12, 16, U8, tp, 2, cp, 3, 1.0),
                 (mp, sp, 12, 16, hiplib.MI_F32, tp, 2, cp, 3, 1.0), (mp, sp, 12, 16, 99, tp, 2, cp, 3, 1.0),
                 (mp, sp, 0, 16, U8, tp, 2, cp, 3, 1.0), (mp, sp, 12, 0, U8, tp, 2, cp, 3, 1.0), (mp, sp, 12, 16, U8, None, 2, cp, 3, 1.0),
                 (mp, sp, 12, 16, U8, tp, 1, cp, 3, 1.0), (mp, sp, 12, 16, U8, tp, 501, cp, 3, 1.0), (mp, sp, 12, 16, U8, tp, -2, cp, 3, 1.0),
                 (mp, sp, 12, 16, U8, tp, 2, None, 3, 1.0), (mp, sp, 12, 16, U8, tp, 2, cp, -1, 1.0), (mp, sp, 12, 16, U8, tp, 2, cp, 65537, 1.0),
                 (mp, sp, 12, 16, U8, tp, 2, cp, 3, 1.5), (mp, sp, 12, 16, U8, tp, 2, cp, 3, -0.1), (mp, sp, 12, 16, U8, tp, 2, cp, 3, float("nan"))):
        assert both(*args) == (INV, INV), args
        assert lib.mi_last_error()
    # the device form's box stays inside the frame
    assert lib.mi_brush_stroke_device(0, None, mp, sp, 12, 16, U8, tp, 2, cp, 3, None, 1.0, None) == INV
    for bad_box in ([-1, 0, 16, 12], [0, -1, 16, 12], [0, 0, 17, 12], [0, 0, 16, 13]):
        b = np.array(bad_box, np.int32)
        assert lib.mi_brush_stroke_device(0, None, mp, sp, 12, 16, U8, tp, 2, cp, 3, b.ctypes.data, 1.0, None) == INV, bad_box
    mask = np.zeros((12, 16))
    kp = mask.ctypes.data
    for args in ((None, sp, kp, 12, 16, U8, 1.0), (mp, None, kp, 12, 16, U8, 1.0), (mp, sp, None, 12, 16, U8, 1.0), (mp, mp, kp, 12, 16, U8, 1.0),
                 (mp, sp, kp, 12, 16, hiplib.MI_F32, 1.0), (mp, sp, kp, 0, 16, U8, 1.0), (mp, sp, kp, 12, 0, U8, 1.0), (mp, sp, kp, 12, 16, U8, 2.0),
                 (mp, sp, kp, 12, 16, U8, float("nan"))):
        assert lib.mi_blend_mask(0, *args) == INV, args
        assert lib.mi_blend_mask_device(0, None, *args) == INV, args
    assert (retouch.MIN_RADIUS, retouch.MAX_RADIUS, retouch.MAX_STAMPS) == (2, 500, 65536)
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "shinestacker_amd", "csrc", "kernels_brush.hpp")).read()
    for name, v in (("MI_BR_MIN_RADIUS", 2), ("MI_BR_MAX_RADIUS", 500), ("MI_BR_MAX_STAMPS", 65536)):
        assert f"#define {name} {v}\n" in text


# ------------------------------------------------------------------ actions and pipeline, as far as no device is needed
def test_focus_stack_without_retouch_leaves_the_golden_trace_unchanged(oracle, tmp_path):
    from shinestacker_amd import FocusStack, StackJob
    from shinestacker_amd.imageio import read_img
    from test_host_logic import OracleStacker, normalise, recorder
    work = str(tmp_path)
    os.makedirs(tmp_path / "input")
    for n in sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop"))):
        shutil.copy(os.path.join(GOLDEN, "img_jpg_crop", n), tmp_path / "input" / n)
    with open(os.path.join(GOLDEN, "plumbing.json")) as fh:
        gold = json.load(fh)
    trace, cbs = recorder()
    job = StackJob("job", work, input_path="input", callbacks=cbs)
    action = FocusStack("stack-pyramid", OracleStacker(oracle), output_path="out-stack", prefix="pyr_", retouch=None)
    messages = []
    action.sub_message_r = lambda msg, *a, **k: messages.append(msg)
    job.add_action(action)
    job.run()
    assert action.retouch is None and not any("retouch" in m for m in messages)
    assert normalise(trace, work) == normalise(gold["trace_stack"], work)
    out = read_img(os.path.join(work, "out-stack", gold["stack_out_files"][0]))
    assert np.array_equal(out, load_golden("plumbing_outputs")["stack"])


def test_actions_and_pipeline_check_the_retouch_option():
    from shinestacker_amd import FocusStack, FocusStackBunch, PyramidStack, pipeline
    st = Stroke(1, [(3, 3)])
    a = FocusStack("stack", PyramidStack(), retouch=[st, Stroke("0002.png", [(4, 4)], 9)])
    assert a.retouch[0] is st and a.retouch[1].source == "0002.png"
    assert FocusStack("stack", PyramidStack()).retouch is None
    for bad in ([(1, [(3, 3)])], 7, [st, None]):
        with pytest.raises(InvalidOptionError):
            FocusStack("stack", PyramidStack(), retouch=bad)
    with pytest.raises(InvalidOptionError):
        FocusStackBunch("bunch", PyramidStack(), retouch=[st])
    assert FocusStackBunch("bunch", PyramidStack(), retouch=None).retouch is None
    par = inspect.signature(pipeline.align_and_stack).parameters
    assert par["retouch"].default is None
    assert "retouch" not in inspect.signature(pipeline.align_and_stack_device).parameters
    assert "retouch" in pipeline.align_and_stack_device.__doc__
    par = inspect.signature(pipeline._finish).parameters
    assert par["on_fused_frame"].default is None
    fr = [np.zeros((40, 60, 3), np.uint8)] * 2
    for bad in ([Stroke(2, [(3, 3)])], [Stroke(-1, [(3, 3)])], [Stroke("0000.png", [(3, 3)])], [3], 3):
        with pytest.raises(InvalidOptionError):
            pipeline.align_and_stack(fr, retouch=bad)
    assert pipeline._check_brush(None, 2) is None and pipeline._brush_paint(None, {}, 4, 4, np.uint8, 0) is None
    assert pipeline._brush_paint([], {}, 4, 4, np.uint8, 0) is None


def test_package_exports_the_module():
    import shinestacker_amd as sa
    assert sa.retouch is retouch and "retouch" in sa.__all__ and sa.Stroke is retouch.Stroke and "Stroke" in sa.__all__
    for name in ("brush_mask", "stamps_along", "stroke", "stroke_device", "apply", "apply_device", "blend", "blend_device"):
        assert callable(getattr(retouch, name))
