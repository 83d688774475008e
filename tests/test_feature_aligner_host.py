"""CPU: the cases of tests/test_gpu_feature_aligner.py run through tests/features_restatement.py, so that none of them is
vacuous -- which truncate at n_level, which move the cut, which leave a level with one train descriptor or none, which meet
RANSAC count ties -- the area sub-sampling by hand on a 4 x 4 frame, and what the Python layer refuses, with its texts."""
import numpy as np
import pytest

import feature_aligner_cases as ac
import features_cases as fc
import features_restatement as fr

from shinestacker_amd import align, features as ft, pipeline
from shinestacker_amd.errors import InvalidOptionError


# ------------------------------------------------------------------------------------------------ selection
def test_selection_cases_do_what_their_names_say():
    stats = {name: ac.level_stats(*case) for name, case in ac.selection_cases().items()}
    cap8 = fr.capacity(8)
    assert stats["none"] == [(True, 21, 0, 0)] and stats["one"] == [(True, 21, 1, 1)]
    assert stats["exactly_n"] == [(True, 21, 8, 8)]                       # as many candidates as n_level
    assert stats["n_plus_one"] == [(True, 21, 9, 8)]                      # one more: truncated
    _, cut, n_sel, kept = stats["one_score_raster"][0]
    assert cut == 21 and n_sel > 8 == kept                                # one score: the raster order alone decides
    kp, _ = fr.extract(*ac.selection_cases()["one_score_raster"])
    assert len(set(kp[:, 3].tolist())) == 1 and kp[:, :2].tolist() == [[18 + 12 * i, 18] for i in range(8)]
    _, cut, n_sel, kept = stats["cut_rises"][0]
    assert cut > 21 and 8 < n_sel <= cap8 and kept == 8                   # more corners than the capacity: the cut moves up
    frame = ac.selection_cases()["cut_rises"][0]
    assert np.count_nonzero(fr.score_plane(frame, 20)[0]) > cap8
    assert stats["one_class_overflows"][0][1:] == (226, 0, 0)             # one score class over the capacity: nothing is kept
    # the LDS bound itself: exactly as many candidates as sixteen thousand keys, and n_level of them kept
    assert stats["lds_bound"] == [(True, 21, 16384, 4096)] and fr.capacity(4096) == 16384
    assert [s[0] for s in stats["third_level_too_small"]] == [True, True, False]
    assert all(s[3] > 0 for s in stats["third_level_too_small"][:2])
    assert stats["side_33"] == [(True, 190, 1, 1)] or stats["side_33"][0][3] == 1    # the smallest side that scores: one pixel
    assert [s[3] for s in stats["scene_truncates"]] == [100, 50, 25]
    assert all(s[2] > s[3] for s in stats["scene_truncates"])             # every level truncates
    assert all(s[2] == s[3] > 0 for s in stats["scene_l3"])               # none does


def test_area_subsampling_by_hand():
    f = np.array([[[0, 1, 2], [3, 4, 5], [10, 20, 30], [11, 21, 31]],
                  [[1, 1, 1], [2, 2, 2], [12, 22, 32], [13, 23, 33]],
                  [[255, 255, 255], [255, 255, 255], [0, 0, 0], [0, 0, 1]],
                  [[255, 255, 255], [254, 255, 255], [0, 0, 0], [0, 0, 0]]], np.uint8)
    want = np.array([[[2, 2, 3], [12, 22, 32]], [[255, 255, 255], [0, 0, 0]]], np.uint8)      # (6+2)>>2, (8+2)>>2, (10+2)>>2; ...
    assert np.array_equal(ac.subsample_area2(f), want)
    assert np.array_equal(align.img_subsample(f, 2, False), want)
    g = fr.gray(want)
    assert g.tolist() == [[(2 * 1868 + 2 * 9617 + 3 * 4899 + 8192) >> 14, (12 * 1868 + 22 * 9617 + 32 * 4899 + 8192) >> 14], [255, 0]]
    # sixteen bits: the mean is taken of the samples, the low byte goes afterwards
    f16 = np.array([[[0x01FF], [0x01FF]], [[0x01FF], [0x0203]]], np.uint16).repeat(3, axis=2)
    assert align.img_subsample(f16, 2, False)[0, 0, 0] == 0x0200 and fr.gray(align.img_subsample(f16, 2, False))[0, 0] == 2
    assert fr.gray(f16)[0, 0] == 1
    for name, (frame, s, fast) in ac.gray_cases().items():
        sub = align.img_subsample(frame, s, fast)
        assert sub.shape[:2] == ((-(-frame.shape[0] // s), -(-frame.shape[1] // s)) if fast or s == 1 else
                                 (frame.shape[0] // 2, frame.shape[1] // 2)), name
        if s == 2 and not fast:
            assert np.array_equal(sub, ac.subsample_area2(frame)), name


# ------------------------------------------------------------------------------------------------ matches and RANSAC
def test_one_sided_pairs_are_one_sided():
    mov, ref = ac.level_in_one_frame_only()
    k0, _ = fr.extract(mov, 3, 200, 20)
    k1, _ = fr.extract(ref, 3, 200, 20)
    assert (np.bincount(k0[:, 2], minlength=3) > 0).all()
    assert (np.bincount(k1[:, 2], minlength=3) > 0).tolist() == [True, True, False]      # a level the reference lacks
    mov, ref = ac.one_train_pair()
    assert len(fr.extract(ref, 3, 200, 20)[0]) == 1 and len(fr.extract(mov, 3, 200, 20)[0]) == 5      # nt == 1 on level 0
    assert len(fr.extract(ac.blank(64, 160), 3, 200, 20)[0]) == 0
    want = ac.expected_pair(mov, ref, 3, 200, 20, "KNN", 0.75, fr.SIMILARITY, 3.0, 8, 0)
    assert len(want["good"]) == 5 and (want["good"][:, 1] == 0).all()      # 0xFFFF as the second distance passes the ratio test
    assert len(ac.expected_pair(mov, ref, 3, 200, 20, "NORM_HAMMING", 0.75, fr.SIMILARITY, 3.0, 8, 0)["good"]) == 1


def test_few_match_cases_meet_ties_and_degenerate_tables():
    for name, (mov, ref, n, method, kind, what) in ac.few_match_cases().items():
        want = ac.expected_pair(mov, ref, 1, n, 20, method, 0.75, kind, 3.0, 32, 5)
        if what == "too_few":
            assert len(want["good"]) == 2 < ac.NEED[kind] and want["samples"] is None
        elif what == "tie":
            assert len(want["good"]) == n and (want["counts"] == n).all() and want["winner"] == 0      # 32 hypotheses tie
            assert all(len(set(r)) == ac.SAMPLE[kind] for r in want["samples"].tolist())
        else:
            assert len(want["good"]) >= 4 and (want["counts"] == -1).all() and want["winner"] == -1 and want["m"] is None
    assert len(ac.expected_pair(*ac.few_match_cases()["n_equals_m"][:2], 1, 4, 20, "NORM_HAMMING", 0.75, fr.HOMOGRAPHY, 3.0, 4,
                                5)["good"]) == ac.SAMPLE[fr.HOMOGRAPHY]      # n == m: every row a permutation of all matches


def test_sample_table_of_the_product_equals_the_restatement_at_the_sizes_used():
    for n, k, m, seed in ((4, 32, 4, 5), (3, 32, 2, 5), (2, 7, 2, 0), (130, 300, 2, 0), (130, 300, 4, 0)):
        assert np.array_equal(ft.sample_table(n, k, m, seed), fr.sample_table(n, k, m, seed))


def test_retry_scene_needs_the_retry():
    frames, _ = ac.pipeline_frames()
    weak, _ = ac.retry_frame()
    ref = frames[3]
    n2 = fr.estimate(align.img_subsample(weak, 2, False), align.img_subsample(ref, 2, False))[0]
    n1, m1 = fr.estimate(weak, ref)
    assert n2 <= ac.RETRY_MIN_GOOD < n1 and m1 is not None
    for i, f in enumerate(frames):
        if i != 3:
            assert fr.estimate(align.img_subsample(f, 2, False), align.img_subsample(ref, 2, False))[0] > ac.RETRY_MIN_GOOD, i
    assert fr.estimate(ac.blank(240, 320), ref)[0] == 0


# ------------------------------------------------------------------------------------------------ what is refused
def test_refusal_texts():
    with pytest.raises(InvalidOptionError, match="fast_subsampling=True"):
        ft.check_subsampling(240, 320, 3, False)
    with pytest.raises(InvalidOptionError, match="fast_subsampling=True"):
        ft.check_subsampling(241, 320, 2, False)
    with pytest.raises(InvalidOptionError, match="fast_subsampling=True"):
        ft.check_subsampling(240, 321, 2, False)
    with pytest.raises(InvalidOptionError):
        ft.check_subsampling(240, 320, 0, True)
    assert ft.check_subsampling(241, 321, 3, True) == 3 and ft.check_subsampling(240, 320, 2, False) == 2
    assert ft.check_subsampling(241, 321, 1, False) == 1
    with pytest.raises(InvalidOptionError, match="fits with RANSAC only"):
        ft.FeatureAligner.options({}, {"align_method": "LMEDS"})
    with pytest.raises(InvalidOptionError):
        ft.FeatureAligner.options({}, {"transform": "ALIGN_AFFINE"})
    with pytest.raises(InvalidOptionError, match="Valid options are"):
        ft.FeatureAligner.options({"match_method": "FLANN"}, {})
    for bad in (0, 4097, 2.5, True):
        with pytest.raises(InvalidOptionError, match="max_iters"):
            ft.FeatureAligner.options({}, {"max_iters": bad})
    assert ft.FeatureAligner.options(None, None) == (0, 0.75, ft.SIMILARITY, "ALIGN_RIGID", 3.0, 2000)
    assert ft.FeatureAligner.options({"match_method": "NORM_HAMMING", "threshold": 0.6},
                                     {"transform": "ALIGN_HOMOGRAPHY", "rans_threshold": 2.0, "max_iters": 4096}) == \
        (1, 0.6, ft.HOMOGRAPHY, "ALIGN_HOMOGRAPHY", 2.0, 4096)
    with pytest.raises(InvalidOptionError, match="4096"):
        ft.FeatureAligner(240, 320, np.uint8, ft.FeatureParams(3, 4097, 20))
    with pytest.raises(InvalidOptionError, match="fast_subsampling=True"):
        ft.FeatureAligner(240, 320, np.uint8, subsample=4, fast=False)


def test_pipeline_refuses_before_anything_is_allocated():
    """every combination is refused on a box without a GPU too: nothing has been allocated, no device looked for"""
    def call(**kw):
        return pipeline.align_and_stack_device(0x1000, 4, 240, 320, np.uint8, **kw)
    with pytest.raises(InvalidOptionError, match="Valid options are: None, 'ecc', 'features'"):
        call(estimator="opencv")
    with pytest.raises(InvalidOptionError, match="step_process=True is not implemented with estimator='features'"):
        call(estimator="features", step_process=True)
    with pytest.raises(InvalidOptionError, match="handle reuse"):
        call(estimator="features", keep_handles=True)
    with pytest.raises(InvalidOptionError, match="handle reuse"):
        call(estimator="features", handles=object())
    with pytest.raises(InvalidOptionError, match="fits with RANSAC only"):
        call(estimator="features", alignment_config={"align_method": "LMEDS"})
    with pytest.raises(InvalidOptionError, match="fast_subsampling=True"):
        call(estimator="features", alignment_config={"subsample": 4})
    with pytest.raises(InvalidOptionError, match="max_iters"):
        call(estimator="features", alignment_config={"max_iters": 5000})
    with pytest.raises(InvalidOptionError, match="at most 4096"):
        call(estimator="features", feature_params=ft.FeatureParams(3, 5000, 20))
    with pytest.raises(InvalidOptionError, match="Valid options are"):
        call(estimator="features", matching_config={"match_method": "FLANN"})
