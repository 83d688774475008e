"""GPU: the feature estimator (csrc/kernels_features.hpp) against tests/features_restatement.py, stage by stage and end to
end.  Everything is compared with array_equal except RANSAC's models and the final transform, which are float64 in the same
order of operations (in fact expected identical) and held to rtol 1e-9: eps times the condition cap of 1e6 that
test_features_host.py checks the cases for, with room to spare."""
import numpy as np
import pytest

import features_cases as fc
import features_restatement as fr

from shinestacker_amd import features as ft

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ grey, score, histogram
def test_gray_matches_the_restatement():
    rng = np.random.default_rng(0)
    for shape in ((37, 53, 3), (37, 53), (1, 1, 3), (64, 256)):
        for dt, hi in ((np.uint8, 256), (np.uint16, 65536)):
            a = rng.integers(0, hi, shape).astype(dt)
            assert np.array_equal(ft.gray(a), fr.gray(a)), (shape, dt)
    sat = np.full((5, 7, 3), 65535, np.uint16)
    assert (ft.gray(sat) == 255).all()


@pytest.mark.parametrize("shape", fc.score_shapes(ft.TILE_H, ft.TILE_W), ids=lambda s: f"{s[0]}x{s[1]}")
def test_score_plane_and_histogram(shape):
    h, w = shape
    frames = {"saturated": np.full((h, w), 255, np.uint8), "checkerboard": fc.checkerboard(h, w),
              "random": fc.random_gray(h, w, 5)}
    if shape == (33, 33):
        one = np.full((h, w), 10, np.uint8)
        one[16, 16] = 200
        frames["one_pixel"] = one
    for name, g in frames.items():
        for thr in (20, 0, 254):
            want_s, want_h = fr.score_plane(g, thr)
            got_s, got_h = ft.score(g, thr)
            assert np.array_equal(got_s, want_s), (name, thr)
            assert np.array_equal(got_h, want_h), (name, thr)
    if shape == (33, 33):
        assert ft.score(frames["one_pixel"])[0][16, 16] == 190


# ------------------------------------------------------------------------------------------------ extract
@pytest.mark.parametrize("name", list(fc.extract_cases()))
def test_extract(name):
    img, levels, n, thr, what = fc.extract_cases()[name]
    want_kp, want_desc = fr.extract(img, levels, n, thr)
    got = ft.detect_and_compute(img, ft.FeatureParams(levels, n, thr))
    assert got.kp.dtype == np.int32 and got.desc.dtype == np.uint8 and got.desc.shape == (len(got.kp), 32)
    assert np.array_equal(got.kp, want_kp)
    assert np.array_equal(got.desc, want_desc)
    if what == "none" or what == "short":
        assert len(got.kp) == 0


def test_extract_uint16_equals_its_high_bytes():
    a, b = fc.extract_cases()["bgr_u8_l3"], fc.extract_cases()["bgr_u16_l3"]
    fa, fb = ft.detect_and_compute(a[0]), ft.detect_and_compute(b[0])
    assert len(fa.kp) > 0 and np.array_equal(fa.kp, fb.kp) and np.array_equal(fa.desc, fb.desc)


# ------------------------------------------------------------------------------------------------ match
MATCH_SIZES = sorted({1, 2, 63, 64, 65, ft.MATCH_CHUNK - 1, ft.MATCH_CHUNK, ft.MATCH_CHUNK + 1})


@pytest.fixture(scope="module")
def descriptors():
    rng = np.random.default_rng(4)
    base = rng.integers(0, 256, (ft.MATCH_CHUNK + 1, 32), dtype=np.uint8)
    # near copies, so that best and second best are close and often tied
    other = base ^ (rng.random(base.shape) < 0.03).astype(np.uint8) * rng.integers(0, 256, base.shape, dtype=np.uint8)
    return base, other


@pytest.mark.parametrize("nt", MATCH_SIZES)
def test_match_sizes(descriptors, nt):
    base, other = descriptors
    for nq in MATCH_SIZES:
        q, t = other[:nq], base[:nt]
        assert np.array_equal(ft.match_descriptors(q, t), fr.match_level(q, t)), (nq, nt)


def test_match_special_values(descriptors):
    base, _ = descriptors
    dup = np.concatenate([base[:40], base[:40], base[:40]])
    got = ft.match_descriptors(base[:40], dup)
    assert np.array_equal(got, fr.match_level(base[:40], dup))
    assert np.array_equal(got[:, 0], np.arange(40)) and (got[:, 1] == 0).all() and (got[:, 2] == 0).all()   # lowest index
    zeros, ones = np.zeros((3, 32), np.uint8), np.full((2, 32), 255, np.uint8)
    assert ft.match_descriptors(zeros, ones).tolist() == [[0, 256, 256]] * 3
    assert ft.match_descriptors(zeros, ones[:1]).tolist() == [[0, 256, 0xFFFF]] * 3                          # no second
    far = ft.MATCH_CHUNK + 1
    t = np.full((far, 32), 255, np.uint8)
    t[-1] = 0                                                   # the best lies in the second LDS chunk
    assert ft.match_descriptors(zeros, t).tolist() == [[far - 1, 0, 256]] * 3


# ------------------------------------------------------------------------------------------------ RANSAC
@pytest.mark.parametrize("name, kind, n, k, seed", fc.RANSAC_CASES, ids=[c[0] for c in fc.RANSAC_CASES])
def test_ransac(name, kind, n, k, seed):
    src, dst, samples = fc.ransac_case(kind, n, k, seed)
    want_c, want_m = fr.ransac(src, dst, samples, kind, fc.RANSAC_THR)
    got_c, got_m = ft.ransac(src, dst, samples, kind, fc.RANSAC_THR)
    print(name, "models identical:", np.array_equal(got_m, want_m), "largest relative difference",
          float(np.max(np.abs(got_m - want_m) / np.maximum(np.abs(want_m), 1e-300))))
    assert np.array_equal(got_c, want_c)
    np.testing.assert_allclose(got_m, want_m, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("kind", [fr.SIMILARITY, fr.HOMOGRAPHY])
def test_ransac_degenerate_samples(kind):
    src, dst, samples = fc.degenerate_case(kind)
    want_c, want_m = fr.ransac(src, dst, samples, kind, fc.RANSAC_THR)
    got_c, got_m = ft.ransac(src, dst, samples, kind, fc.RANSAC_THR)
    assert got_c.tolist() == want_c.tolist() and (got_c == -1).tolist() == [True, False, True]
    assert not got_m[got_c == -1].any()
    np.testing.assert_allclose(got_m, want_m, rtol=1e-9, atol=0.0)


def test_find_transform_equals_the_restatement():
    for kind, transform in ((fr.SIMILARITY, "ALIGN_RIGID"), (fr.HOMOGRAPHY, "ALIGN_HOMOGRAPHY")):
        src, dst = fc.ransac_points(kind, 300, 21)
        want_m, want_mask = fr.find_transform(src, dst, kind, 3.0, 500, seed=5)
        got_m, got_mask = ft.find_transform(src, dst, transform, 3.0, 500, seed=5)
        assert got_m.shape == want_m.shape and np.array_equal(got_mask, want_mask) and got_mask.shape == (300, 1)
        np.testing.assert_allclose(got_m, want_m, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def scenes():
    return {"ALIGN_RIGID": fc.scene_similarity(), "ALIGN_HOMOGRAPHY": fc.scene_homography()}


@pytest.mark.parametrize("transform", ["ALIGN_RIGID", "ALIGN_HOMOGRAPHY"])
@pytest.mark.parametrize("method", ["NORM_HAMMING", "KNN"])
def test_align_images_with_the_feature_estimator(scenes, transform, method):
    from shinestacker_amd.align import align_images, apply_transform, _DEFAULT_ALIGNMENT_CONFIG
    h, w, m_true, mov, ref = scenes[transform]
    kind = fr.HOMOGRAPHY if transform == "ALIGN_HOMOGRAPHY" else fr.SIMILARITY
    # (the reference refuses SIFT with Hamming matching and ORB with KNN whichever estimator runs: name a pair it accepts)
    fcfg = {"detector": "ORB", "descriptor": "ORB"} if method == "NORM_HAMMING" else {"detector": "SIFT", "descriptor": "SIFT"}
    acfg = {"transform": transform, "subsample": 1, "max_iters": 500}
    n_good, m, warp = align_images(ref, mov, feature_config=fcfg, matching_config={"match_method": method},
                                   alignment_config=acfg, estimator="features")
    want_n, want_m = fr.estimate(mov, ref, method, 0.75, kind, 3.0, 500, seed=0)
    assert n_good == want_n and n_good >= 100
    np.testing.assert_allclose(m, want_m, rtol=1e-9, atol=1e-12)
    assert fc.corner_error(m, m_true, h, w) <= 1.0
    assert warp is not None and warp.shape == mov.shape and warp.dtype == mov.dtype
    assert np.array_equal(warp, apply_transform(mov, m, {**_DEFAULT_ALIGNMENT_CONFIG, **acfg}))
    # the warp brings the moving frame onto the reference: away from the border the two differ by noise and resampling only
    d = np.abs(warp[20:-20, 20:-20].astype(int) - ref[20:-20, 20:-20].astype(int))
    d0 = np.abs(mov[20:-20, 20:-20].astype(int) - ref[20:-20, 20:-20].astype(int))
    assert d.mean() < 0.5 * d0.mean()


def test_align_images_retries_without_subsampling_on_few_matches(scenes):
    """n_good carries information now: a frame pair that yields few matches when sub-sampled is estimated again at full size"""
    from shinestacker_amd.align import align_images
    h, w, m_true, mov, ref = scenes["ALIGN_RIGID"]
    seen = []
    n_good, m, _ = align_images(ref, mov, alignment_config={"subsample": 4, "fast_subsampling": True, "min_good_matches": 100},
                                estimator="features", callbacks={"warning": seen.append})
    assert len(seen) == 1 and "retrying without subsampling" in seen[0]
    assert n_good == fr.estimate(mov, ref)[0] > 100


def test_align_frames_over_three_frames(scenes):
    from shinestacker_amd.align import AlignFrames
    h, w, m_true, mov, ref = scenes["ALIGN_RIGID"]
    m2 = fc.similarity(-1.0, 0.99, -2.0, 3.0, h, w)
    mov2, _ = fc.pair(h, w, m2, 11)
    frames = [mov, ref, mov2]

    class Process:
        filenames = ["a", "b", "c"]
        ref_idx = 1

        def img_ref(self, idx):
            return frames[idx]

        def sub_message_r(self, msg):
            pass

        def sub_message(self, msg, level=None):
            pass
    step = AlignFrames(estimator="features", alignment_config={"subsample": 1})
    step.begin(Process())
    out = [step.run_frame(i, 1, f) for i, f in enumerate(frames)]
    assert out[1] is ref and all(o.shape == ref.shape for o in out)
    assert step.n_matches[1] == 0 and step.n_matches[0] == fr.estimate(mov, ref)[0] and step.n_matches[2] == fr.estimate(mov2, ref)[0]
    for o, f in ((out[0], mov), (out[2], mov2)):
        d = np.abs(o[20:-20, 20:-20].astype(int) - ref[20:-20, 20:-20].astype(int)).mean()
        assert d < 0.5 * np.abs(f[20:-20, 20:-20].astype(int) - ref[20:-20, 20:-20].astype(int)).mean()
