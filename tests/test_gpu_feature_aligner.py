"""GPU: the resident feature estimator (features.FeatureAligner, mi_feat_aligner_t) against tests/features_restatement.py,
stage by stage through the handle's taps, and against the per-pair host form (features.feature_estimator).  Everything up to
the sample tables and RANSAC's counts is compared with array_equal; RANSAC's models and the final transforms are float64 in
the restatement's order of operations and held to rtol 1e-9, the tolerance tests/test_gpu_features.py uses for them, and to
array_equal against the host form, which runs the same kernels and the same NumPy refit."""
import contextlib

import numpy as np
import pytest

import feature_aligner_cases as ac
import features_cases as fc
import features_restatement as fr

from shinestacker_amd import _lib, align, features as ft, pipeline
from shinestacker_amd.errors import AlignmentError

pytestmark = pytest.mark.gpu

KIND_NAME = {fr.SIMILARITY: "ALIGN_RIGID", fr.HOMOGRAPHY: "ALIGN_HOMOGRAPHY"}


@contextlib.contextmanager
def handle(ref, movs, params=None, subsample=1, fast=True, max_batch=None, seed=0):
    """a FeatureAligner with `ref` set and the frames resident: yields (handle, device addresses of the moving frames)"""
    ref = np.ascontiguousarray(ref)
    frames = [ref] + [np.ascontiguousarray(m) for m in movs]
    assert all(f.shape == ref.shape and f.dtype == ref.dtype for f in frames)
    buf = _lib.DeviceBuffer(ref.nbytes * len(frames))
    fa = None
    try:
        for i, f in enumerate(frames):
            buf.upload(f, i * ref.nbytes)
        fa = ft.FeatureAligner(ref.shape[0], ref.shape[1], ref.dtype, params, subsample=subsample, fast=fast,
                               max_batch=max_batch or max(1, len(movs)), seed=seed, channels=1 if ref.ndim == 2 else 3)
        fa.set_reference(buf.ptr)
        yield fa, [buf.ptr + (i + 1) * ref.nbytes for i in range(len(movs))]
    finally:
        if fa is not None:
            fa.close()
        buf.free()


def cfgs(method="KNN", kind=fr.SIMILARITY, k=200, ratio=0.75, thr=3.0):
    return {"match_method": method, "threshold": ratio}, {"transform": KIND_NAME[kind], "rans_threshold": thr, "max_iters": k}


def check_extraction(fa, slot, frame_sub, p):
    """the taps of one frame against the restatement's extraction of the (sub-sampled) frame"""
    g = fr.gray(frame_sub)
    assert np.array_equal(fa.tap(slot, _lib.FEAT_TAP_GRAY), g)
    for lv, lg in enumerate(fr.pyramid(g, p.levels)):
        assert np.array_equal(fa.tap(slot, _lib.FEAT_TAP_GRAY, lv), lg), lv
    stats = ac.level_stats(frame_sub, p.levels, p.n_features, p.threshold)
    cut = fa.tap(slot, _lib.FEAT_TAP_CUT)
    for lv in range(p.levels):
        want = stats[lv] if lv < len(stats) else (False, 0, 0, 0)
        assert cut[lv].tolist() == ([want[1], want[2], want[3], 0] if want[0] else [0, 0, 0, 0]), (lv, cut[lv], want)
    kp, desc = fr.extract(frame_sub, p.levels, p.n_features, p.threshold)
    assert np.array_equal(fa.tap(slot, _lib.FEAT_TAP_KP), kp)
    assert np.array_equal(fa.tap(slot, _lib.FEAT_TAP_DESC), desc)
    return kp


def check_pair(fa, slot, raw, want, kind, k):
    """one frame's matches, sample table, counts and winner against `ac.expected_pair`"""
    assert np.array_equal(fa.tap(slot, _lib.FEAT_TAP_GOOD), want["good"])
    assert raw["n_good"] == len(want["good"])
    assert np.array_equal(raw["src"], want["src"]) and np.array_equal(raw["dst"], want["dst"])
    if want["samples"] is None:
        assert raw["winner"] == -1 and not raw["model"].any() and raw["inliers"] == 0 and not raw["mask"].any()
        return
    assert np.array_equal(fa.tap(slot, _lib.FEAT_TAP_SAMPLES), want["samples"])
    assert np.array_equal(fa.tap(slot, _lib.FEAT_TAP_SAMPLES), ft.sample_table(raw["n_good"], k, ac.SAMPLE[kind], fa.seed))
    assert np.array_equal(fa.tap(slot, _lib.FEAT_TAP_COUNTS), want["counts"])
    assert raw["winner"] == want["winner"]
    if want["winner"] >= 0:
        np.testing.assert_allclose(raw["model"], want["models"][want["winner"]], rtol=1e-9, atol=0.0)
        assert raw["inliers"] == want["counts"][want["winner"]] == raw["mask"].sum()


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("name", list(ac.selection_cases()))
def test_selection(name):
    frame, levels, n, thr = ac.selection_cases()[name]
    p = ft.FeatureParams(levels, n, thr)
    with handle(frame, [frame], p) as (fa, ptrs):
        raw = fa.estimate_raw(ptrs, *cfgs())
        kp = check_extraction(fa, -1, frame, p)
        assert np.array_equal(check_extraction(fa, 0, frame, p), kp)
        if name == "lds_bound":
            assert fa.tap(0, _lib.FEAT_TAP_CUT)[0].tolist() == [21, 16384, 4096, 0]      # the capacity exactly: 128 KiB of keys
        if len(kp) == 0:
            assert raw[0]["n_good"] == 0 and raw[0]["winner"] == -1


def test_selection_leaves_what_mi_feat_extract_leaves():
    frame, levels, n, thr = ac.selection_cases()["scene_truncates"]
    p = ft.FeatureParams(levels, n, thr)
    with handle(frame, [], p) as (fa, _):
        host = ft.detect_and_compute(frame, p)
        assert np.array_equal(fa.tap(-1, _lib.FEAT_TAP_KP), host.kp) and np.array_equal(fa.tap(-1, _lib.FEAT_TAP_DESC), host.desc)


# ------------------------------------------------------------------------------------------------ grey
@pytest.mark.parametrize("name", list(ac.gray_cases()))
def test_gray_with_subsampling(name):
    frame, s, fast = ac.gray_cases()[name]
    with handle(frame, [frame], ft.FeatureParams(1, 8, 20), subsample=s, fast=fast) as (fa, ptrs):
        fa.estimate_raw(ptrs, *cfgs())
        want = fr.gray(align.img_subsample(frame, s, fast))
        assert fa.shape_sub == want.shape
        assert np.array_equal(fa.tap(-1, _lib.FEAT_TAP_GRAY), want) and np.array_equal(fa.tap(0, _lib.FEAT_TAP_GRAY), want)
        if s == 2 and not fast:
            assert np.array_equal(want, fr.gray(ac.subsample_area2(frame)))


# ------------------------------------------------------------------------------------------------ matches, tables, pick
@pytest.fixture(scope="module")
def scenes():
    return {"similarity": fc.scene_similarity(), "homography": fc.scene_homography(), "defocus": fc.scene_defocus()}


@pytest.mark.parametrize("method", ["NORM_HAMMING", "KNN"])
@pytest.mark.parametrize("scene, kind", [("similarity", fr.SIMILARITY), ("homography", fr.HOMOGRAPHY), ("defocus", fr.SIMILARITY)])
def test_scene_every_stage_and_the_transform(scenes, scene, kind, method):
    h, w, m_true, mov, ref = scenes[scene]
    p, k = ft.FeatureParams(), 300
    mcfg, acfg = cfgs(method, kind, k)
    want = ac.expected_pair(mov, ref, p.levels, p.n_features, p.threshold, method, 0.75, kind, 3.0, k, 0)
    with handle(ref, [mov], p) as (fa, ptrs):
        raw = fa.estimate_raw(ptrs, mcfg, acfg)[0]
        check_extraction(fa, 0, mov, p)
        check_pair(fa, 0, raw, want, kind, k)
        n_good, m, frac = fa.estimate_batch(ptrs, mcfg, acfg)[0]
    host_n, host_m = ft.feature_estimator(p)(mov, ref, {}, mcfg, acfg)
    assert n_good == host_n == len(want["good"]) >= 100
    assert np.array_equal(m, host_m)
    np.testing.assert_allclose(m, want["m"], rtol=1e-9, atol=1e-12)
    assert m.shape == ((3, 3) if kind == fr.HOMOGRAPHY else (2, 3)) and 0.0 < frac <= 1.0
    assert fc.corner_error(m, m_true, h, w) <= 1.0


@pytest.mark.parametrize("method", ["NORM_HAMMING", "KNN"])
def test_levels_and_keypoints_that_one_side_lacks(method):
    p, k = ft.FeatureParams(3, 200, 20), 64
    mcfg, acfg = cfgs(method, fr.SIMILARITY, k)
    pairs = {"level_in_one_frame": ac.level_in_one_frame_only(), "level_in_one_frame_swapped": ac.level_in_one_frame_only()[::-1],
             "one_train_descriptor": ac.one_train_pair(), "one_query_descriptor": ac.one_train_pair()[::-1]}
    for name, (mov, ref) in pairs.items():
        want = ac.expected_pair(mov, ref, p.levels, p.n_features, p.threshold, method, 0.75, fr.SIMILARITY, 3.0, k, 0)
        with handle(ref, [mov], p) as (fa, ptrs):
            raw = fa.estimate_raw(ptrs, mcfg, acfg)[0]
            check_pair(fa, 0, raw, want, fr.SIMILARITY, k)
    b = ac.blank(64, 160)
    some = ac.one_train_pair()[0]
    for mov, ref in ((b, some), (some, b), (b, b)):         # no keypoint in the moving frame, in the reference, in both
        with handle(ref, [mov], p) as (fa, ptrs):
            raw = fa.estimate_raw(ptrs, mcfg, acfg)[0]
            assert raw["n_good"] == 0 and raw["winner"] == -1 and not raw["model"].any() and len(raw["mask"]) == 0
            assert fa.estimate_batch(ptrs, mcfg, acfg) == [(0, None, 0.0)]


def test_sample_tables_and_pick_on_few_matches():
    """pairs with a handful of good matches (ac.few_match_cases): too few to fit, a table with n == m, count ties (the lowest
    index wins), and hypotheses that are all degenerate (no winner)"""
    k = 32
    for name, (mov, ref, n, method, kind, what) in ac.few_match_cases().items():
        mcfg, acfg = cfgs(method, kind, k)
        want = ac.expected_pair(mov, ref, 1, n, 20, method, 0.75, kind, 3.0, k, 5)
        with handle(ref, [mov], ft.FeatureParams(1, n, 20), seed=5) as (fa, ptrs):
            raw = fa.estimate_raw(ptrs, mcfg, acfg)[0]
            check_pair(fa, 0, raw, want, kind, k)
            if what in ("too_few", "no_winner"):
                assert raw["winner"] == -1 and fa.estimate_batch(ptrs, mcfg, acfg) == [(raw["n_good"], None, 0.0)], name
            else:
                assert raw["winner"] == 0 and raw["inliers"] == raw["n_good"], name


# ------------------------------------------------------------------------------------------------ batches, structure
def test_batches_equal_single_frames_and_repeat(scenes):
    h, w, _, mov, ref = scenes["similarity"]
    few = ref.copy()
    few[:, 120:] = 90                                        # few keypoints
    movs = [mov, ac.blank(h, w), few, ref, mov[::-1].copy(), ac.blank(h, w), mov, few]
    p, (mcfg, acfg) = ft.FeatureParams(3, 300, 20), cfgs("NORM_HAMMING", fr.SIMILARITY, 100)
    alone = []
    for f in movs[:5]:
        with handle(ref, [f], p) as (fa, ptrs):
            w0, l0 = fa.stats()
            alone.append(fa.estimate_raw(ptrs, mcfg, acfg)[0])
            w1, l1 = fa.stats()
    alone += [alone[1], alone[0], alone[2]]
    assert alone[0]["n_good"] > 50 and alone[1]["n_good"] == 0 and 0 < alone[2]["n_good"]       # many, none, some
    with handle(ref, movs, p, max_batch=len(movs)) as (fa, ptrs):
        wa, la = fa.stats()
        first = fa.estimate_raw(ptrs, mcfg, acfg)
        wb, lb = fa.stats()
        second = fa.estimate_raw(ptrs[::-1], mcfg, acfg)[::-1]      # other slots: nothing of the first batch may show
        third = fa.estimate_raw(ptrs[:1], mcfg, acfg)
    for got in (first, second, third):
        for a, b in zip(got, alone):
            assert a.keys() == b.keys() and all(np.array_equal(a[key], b[key]) for key in a), "a frame in a batch differs from it alone"
    # structure: at most two waits per call, and as many launches for eight frames as for one
    assert w1 - w0 <= 2 and wb - wa <= 2
    assert lb - la == l1 - l0 > 0


def test_call_order_and_tap_range(scenes):
    h, w, _, mov, ref = scenes["similarity"]
    buf = _lib.DeviceBuffer(2 * ref.nbytes)
    fa = None
    try:
        buf.upload(ref)
        buf.upload(mov, ref.nbytes)
        fa = ft.FeatureAligner(h, w, ref.dtype, max_batch=2)
        with pytest.raises(_lib.DeviceError, match="set_reference has not been called"):
            fa.estimate_raw([buf.ptr + ref.nbytes])
        with pytest.raises(_lib.DeviceError, match="set_reference has not been called"):
            fa.tap(-1, _lib.FEAT_TAP_KP)
        fa.set_reference(buf.ptr)
        with pytest.raises(_lib.DeviceError, match="not part of the last batch"):
            fa.tap(0, _lib.FEAT_TAP_KP)
        fa.estimate_raw([buf.ptr + ref.nbytes])
        with pytest.raises(_lib.DeviceError, match="not part of the last batch"):
            fa.tap(1, _lib.FEAT_TAP_KP)
        for slot, what in ((2, _lib.FEAT_TAP_KP), (-2, _lib.FEAT_TAP_KP), (0, 7), (-1, _lib.FEAT_TAP_GOOD)):
            with pytest.raises(ValueError):
                fa.tap(slot, what)
        with pytest.raises(ValueError, match="level"):
            fa.tap(0, _lib.FEAT_TAP_GRAY, 3)
        with pytest.raises(ValueError, match="n must be"):
            fa.estimate_raw([buf.ptr] * 3)
        # estimate_batch's own arguments, each named before any device call
        import ctypes
        lib, hd, cap = _lib.load(), fa._al._h, fa._al.max_matches
        out = np.zeros(cap * 16, np.uint8).ctypes.data
        good = dict(movs=(ctypes.c_void_p * 1)(buf.ptr + ref.nbytes), n=1, method=0, ratio=0.75, kind=0, thr=3.0, k=100, seed=0,
                    cap=cap, n_good=out, winner=out, models=out, inliers=out, mask=out, src=out, dst=out)
        for kw, text in (({"movs": None}, "null frame list"), ({"n": 0}, "n must be in [1, max_batch = 2]"),
                         ({"movs": (ctypes.c_void_p * 1)(None)}, "null frame 0"), ({"method": 2}, "unknown match_method 2"),
                         ({"ratio": 0.0}, "ratio must be finite and > 0"), ({"ratio": float("nan")}, "ratio must be finite"),
                         ({"kind": 2}, "unknown kind 2"), ({"thr": -1.0}, "rans_threshold must be finite and > 0"),
                         ({"thr": float("inf")}, "rans_threshold must be finite"), ({"k": 0}, "max_iters must be in [1, 4096]"),
                         ({"k": 4097}, "max_iters must be in [1, 4096]"), ({"cap": cap - 1}, "max_matches must hold"),
                         ({"n_good": None}, "null n_good"), ({"winner": None}, "null winner"), ({"models": None}, "null models"),
                         ({"inliers": None}, "null inliers"), ({"mask": None}, "null mask"), ({"src": None}, "null src"),
                         ({"dst": None}, "null dst")):
            assert lib.mi_feat_aligner_estimate_batch(hd, *{**good, **kw}.values()) == _lib.MI_ERR_INVALID, kw
            assert text in _lib.last_error(), (kw, _lib.last_error())
        n_out = ctypes.c_int(0)
        assert lib.mi_feat_aligner_tap(hd, 0, _lib.FEAT_TAP_KP, 0, None, 64, ctypes.byref(n_out)) == _lib.MI_ERR_INVALID
        assert lib.mi_feat_aligner_tap(hd, 0, _lib.FEAT_TAP_KP, 0, out, 64, None) == _lib.MI_ERR_INVALID
        assert lib.mi_feat_aligner_tap(hd, 0, _lib.FEAT_TAP_KP, 0, out, 19, ctypes.byref(n_out)) == _lib.MI_ERR_INVALID
        assert "capacity must be at least" in _lib.last_error()
        assert lib.mi_feat_aligner_set_reference(hd, None) == _lib.MI_ERR_INVALID and "null reference frame" in _lib.last_error()
        assert lib.mi_feat_aligner_stats(hd, None, None) == _lib.MI_ERR_INVALID
    finally:
        if fa is not None:
            fa.close()
        buf.free()


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def stack_frames():
    frames, _ = ac.pipeline_frames()
    return frames


def resident(frames, **kw):
    fb = frames[0].nbytes
    buf = _lib.DeviceBuffer(fb * len(frames))
    try:
        for i, f in enumerate(frames):
            buf.upload(f, i * fb)
        h, w = frames[0].shape[:2]
        return pipeline.align_and_stack_device(buf.ptr, len(frames), h, w, frames[0].dtype, **kw)
    finally:
        buf.free()


@pytest.mark.parametrize("sub, fast", [(1, False), (2, False), (2, True)])
def test_pipeline_equals_the_host_estimator(stack_frames, sub, fast):
    frames = stack_frames
    acfg = {"subsample": sub, "fast_subsampling": fast, "max_iters": 300, "min_good_matches": 10}
    mcfg = {"match_method": "KNN"}
    info = {}
    out, transforms, fracs = resident(frames, estimator="features", alignment_config=acfg, matching_config=mcfg, ecc_batch=4,
                                      info=info)
    est = ft.feature_estimator()
    ref, transform = frames[3], align._DEFAULT_ALIGNMENT_CONFIG["transform"]
    for i, f in enumerate(frames):
        if i == 3:
            assert transforms[i] is None and fracs[i] == 1.0 and info["good_matches"][i] == 0
            continue
        a, b = align.img_subsample(f, sub, fast), align.img_subsample(ref, sub, fast)
        n, m = est(a, b, {}, mcfg, {**align._DEFAULT_ALIGNMENT_CONFIG, **acfg})
        if sub > 1:
            m = align.rescale_transform(m, transform, sub, f.shape, a.shape)
        assert info["good_matches"][i] == n > 10 and np.array_equal(transforms[i], m), i
        assert 0.0 < fracs[i] <= 1.0
    assert info["feature_retries"] == []
    want, matches = pipeline.align_and_stack(frames, estimator="features", alignment_config=acfg, matching_config=mcfg)
    assert matches == info["good_matches"]
    assert np.array_equal(out, want)


def test_pipeline_retries_blank_frames_and_leaves_ecc_alone(stack_frames):
    frames = list(stack_frames)
    weak, _ = ac.retry_frame()
    frames[1] = weak
    acfg = {"subsample": 2, "fast_subsampling": False, "max_iters": 300, "min_good_matches": ac.RETRY_MIN_GOOD}
    info = {}
    out, transforms, _ = resident(frames, estimator="features", alignment_config=acfg, info=info)
    assert info["feature_retries"] == [1]
    n2 = fr.estimate(align.img_subsample(weak, 2, False), align.img_subsample(frames[3], 2, False))[0]
    n1 = fr.estimate(weak, frames[3])[0]
    assert n2 <= ac.RETRY_MIN_GOOD < n1 == info["good_matches"][1]
    assert np.array_equal(transforms[1], ft.feature_estimator()(weak, frames[3], {}, {}, {"max_iters": 300})[1])
    want, matches = pipeline.align_and_stack(frames, estimator="features", alignment_config=acfg)
    assert matches == info["good_matches"] and np.array_equal(out, want)
    # a blank frame has no model: AlignmentError with its index
    frames[4] = ac.blank(240, 320)
    with pytest.raises(AlignmentError) as e:
        resident(frames, estimator="features", alignment_config=acfg)
    assert e.value.index == 4
    # without the argument the call is what it was: the ECC estimator
    base = resident(stack_frames)
    ecc = resident(stack_frames, estimator="ecc")
    assert np.array_equal(base[0], ecc[0]) and base[2] == ecc[2]
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(base[1], ecc[1]))
