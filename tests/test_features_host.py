"""CPU: the feature estimator's specification (tests/features_restatement.py) checked by hand on tiny inputs, its cases
checked not to be vacuous, and the host-side parts of shinestacker_amd/features.py held to the restatement.

End to end through the restatement (largest corner error of the recovered transform, pixels; the bound is 1.0 -- RANSAC's own
inlier radius is 3 px and a refit over hundreds of inliers must beat it):
    240 x 320 similarity   NORM_HAMMING 0.162   KNN 0.248
    240 x 320 homography   NORM_HAMMING 0.463   KNN 0.710
    480 x 640 sigma-2 blur NORM_HAMMING 0.742   KNN 0.745
"""
import os
import re
import zlib

import numpy as np
import pytest

import features_cases as fc
import features_restatement as fr
from conftest import ROOT

from shinestacker_amd import align as al
from shinestacker_amd import features as ft
from shinestacker_amd.errors import InvalidOptionError

PATTERN_CRC32 = 2059093025


def test_pattern_is_pinned_and_well_formed():
    p = fr.pattern()
    assert p.shape == (32, 256, 4) and p.dtype == np.int8
    assert zlib.crc32(p.tobytes()) == PATTERN_CRC32
    assert np.abs(p).max() == 13                               # 13 + 2 for the box stays inside the edge of 16
    assert np.abs(fr.base_pattern()).max() <= 9
    assert not (p[0, :, 0:2] == p[0, :, 2:4]).all(axis=1).any()   # no base test compares a point with itself
    assert np.array_equal(p[0], fr.base_pattern())
    assert np.array_equal(ft.pattern(), p) and not ft.pattern().flags.writeable


def test_product_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "shinestacker_amd", "csrc", "kernels_features.hpp")).read()

    def const(name):
        return int(re.search(rf"\b{name} = (\d+)", text).group(1))
    assert (ft.TILE_H, ft.TILE_W, ft.EDGE) == (const("TILE_H"), const("TILE_W"), const("EDGE")) and ft.EDGE == fr.EDGE
    assert (ft.MATCH_NT, ft.MATCH_CHUNK) == (const("MATCH_NT"), const("MATCH_CHUNK"))
    assert (ft.BINS, ft.N_TESTS, ft.NO_SECOND) == (const("BINS"), const("N_TESTS"), fr.NO_SECOND)
    head = open(os.path.join(ROOT, "include", "mi355stack.h")).read()
    assert re.search(r"MI_FEAT_SIMILARITY = 0, MI_FEAT_HOMOGRAPHY = 1", head)
    assert (ft.SIMILARITY, ft.HOMOGRAPHY) == (fr.SIMILARITY, fr.HOMOGRAPHY) == (0, 1)


# ------------------------------------------------------------------------------------------------ by hand
def test_gray_and_pyramid_by_hand():
    img = np.zeros((2, 2, 3), np.uint8)
    img[0, 0] = (255, 0, 0)
    img[0, 1] = (0, 255, 0)
    img[1, 0] = (0, 0, 255)
    img[1, 1] = (255, 255, 255)
    g = fr.gray(img)
    assert g.tolist() == [[29, 150], [76, 255]]                 # (255 * 1868 + 8192) >> 14 = 29, ...
    assert np.array_equal(fr.gray((img.astype(np.uint16) << 8) | 0xFF), g)
    assert fr.halve(g).tolist() == [[(29 + 150 + 76 + 255 + 2) >> 2]]
    assert fr.halve(np.arange(15, dtype=np.uint8).reshape(3, 5)).shape == (1, 2)
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((4,), np.uint8)):
        with pytest.raises(ValueError):
            fr.gray(bad)


def test_single_bright_pixel():
    g = np.full((41, 41), 10, np.uint8)
    g[20, 20] = 200
    s, h = fr.score_plane(g)
    assert s[20, 20] == 190 and np.count_nonzero(s) == 1        # every circle pixel is 190 darker; its neighbours see one
    assert h[190] == 1 and h.sum() == 1                         # bright circle pixel only: no arc of 9
    g[20, 20] = 30                                              # 20 above: not above the threshold of 20
    assert np.count_nonzero(fr.score_plane(g)[0]) == 0
    g[20, 20] = 31
    assert fr.score_plane(g)[0][20, 20] == 21
    g[:] = 10
    g[15, 20] = 200                                             # nearer than 16 to the border: scores 0
    assert np.count_nonzero(fr.score_plane(g)[0]) == 0
    assert np.count_nonzero(fr.score_plane(np.full((32, 40), 10, np.uint8))[0]) == 0


def test_step_corner_has_the_step_as_score():
    g = np.full((41, 41), 50, np.uint8)
    g[20:, 20:] = 150                                           # a two-level corner, its tip at (20, 20)
    raw = fr.raw_score(g)
    assert raw[20, 20] == 100                                   # 11 contiguous circle pixels lie 100 below the tip
    assert raw[21, 21] == 100                                   # 9 of them one step inside: the same score, later in raster order
    s, _ = fr.score_plane(g)
    assert s[20, 20] == 100 and s[21, 21] == 0
    assert raw[19, 19] == 0                                     # outside the corner only 5 circle pixels differ


def test_suppression_tie_pair():
    g = np.full((41, 41), 10, np.uint8)
    g[20, 20] = g[20, 21] = 200
    raw = fr.raw_score(g)
    assert raw[20, 20] == raw[20, 21] == 190
    s, h = fr.score_plane(g)
    assert s[20, 20] == 190 and s[20, 21] == 0 and h[190] == 1  # the first in raster order survives the tie


@pytest.mark.parametrize("sx, sy, want", [(1, 0, 0), (1, 1, 4), (0, 1, 8), (-1, 1, 12), (-1, 0, 16), (-1, -1, 20), (0, -1, 24),
                                          (1, -1, 28)])
def test_orientation_bin_of_a_half_or_quarter_bright_disc(sx, sy, want):
    g = np.full((41, 41), 20, np.uint8)
    y, x = np.mgrid[0:41, 0:41]
    lit = np.ones((41, 41), bool)
    if sx:
        lit &= (x - 20) * sx > 0
    if sy:
        lit &= (y - 20) * sy > 0
    g[lit] = 220
    m10, m01 = fr.moments(g, 20, 20)
    assert (np.sign(m10), np.sign(m01)) == (sx, sy)
    assert fr.orientation_bin(m10, m01) == want
    assert fr.orientation_bins(g, np.array([20]), np.array([20]))[0] == want


def test_selection_by_hand():
    s = np.zeros((40, 40), np.uint8)
    s[5, 7], s[5, 3], s[2, 9], s[8, 1] = 50, 50, 50, 90
    h = np.bincount(s[s > 0], minlength=256)
    assert fr.select_cut(h, 20, 2) == 21
    x, y, sc = fr.select(s, h, 20, 3)
    assert list(zip(sc, y, x)) == [(90, 8, 1), (50, 2, 9), (50, 5, 3)]      # score descending, then y, then x
    h[60] = 5000                                                # a class that overflows the capacity of 4096 alone
    assert fr.select_cut(h, 20, 2) == 61
    assert fr.capacity(8) == 4096 and fr.capacity(2000) == 8000


def test_descriptor_bits_by_hand():
    g = fc.random_gray(48, 48, 3)
    b = fr.box5(g)
    assert b[10, 10] == g[8:13, 8:13].astype(int).sum()
    d = fr.describe(g, np.array([24]), np.array([20]), np.array([5]))
    t = fr.pattern()[5]
    for j in (0, 31, 32, 255):
        bit = b[20 + t[j, 1], 24 + t[j, 0]] < b[20 + t[j, 3], 24 + t[j, 2]]
        assert (d[0, j // 8] >> (j % 8)) & 1 == int(bit)
    assert fr.positions(np.array([[3, 5, 0, 0, 0], [3, 5, 2, 0, 0]])).tolist() == [[3.0, 5.0], [13.5, 21.5]]


def test_match_by_hand():
    q = np.zeros((3, 32), np.uint8)
    t = np.zeros((4, 32), np.uint8)
    t[0, 0], t[1, 0], t[2, :], t[3, 0] = 0x0F, 0x01, 0xFF, 0x01
    q[1, :] = 0xFF
    q[2, 0] = 0x03
    assert fr.match_level(q, t).tolist() == [[1, 1, 1], [2, 0, 252], [1, 1, 1]]      # ties: the lowest index
    assert fr.match_level(q, t[:1]).tolist() == [[0, 4, 0xFFFF], [0, 252, 0xFFFF], [0, 2, 0xFFFF]]
    kq = np.zeros((3, 5), np.int32)
    kt = np.zeros((4, 5), np.int32)
    m = fr.match(kq, q, kt, t, "NORM_HAMMING")
    assert m.tolist() == [[1, 2, 0], [0, 1, 1]]                 # q2 loses t1 to q0 (t1's nearest, lowest index)
    assert fr.match(kq, q, kt, t, "KNN", 0.75).tolist() == [[1, 2, 0]]
    kt[:, 2] = 1                                                # another level: nothing matches
    assert len(fr.match(kq, q, kt, t, "KNN")) == 0


# ------------------------------------------------------------------------------------------------ no case is vacuous
def test_extract_cases_find_what_they_claim():
    for name, (img, levels, n, thr, what) in fc.extract_cases().items():
        kp, desc = fr.extract(img, levels, n, thr)
        assert desc.shape == (len(kp), 32)
        per_level = np.bincount(kp[:, 2], minlength=3) if len(kp) else np.zeros(3, int)
        if what == "some":
            assert all(per_level[lv] > 0 for lv in range(levels)), name
            assert all(per_level[lv] <= n >> lv for lv in range(levels)), name
        elif what == "none":
            assert len(kp) == 0, name
        elif what == "short":
            s, h = fr.score_plane(fr.gray(img), thr)
            assert h.sum() > fr.capacity(n) and per_level[0] < n, name
        elif what == "two_levels":
            assert per_level[0] > 0 and per_level[1] > 0 and per_level[2] == 0, name
    kp, _ = fr.extract(*fc.extract_cases()["dots_n8"][0:4])
    assert len(set(kp[:, 3].tolist())) == 1 and kp[:, :2].tolist() == [[18 + 12 * i, 18] for i in range(8)]
    a, b = fc.extract_cases()["bgr_u8_l3"], fc.extract_cases()["bgr_u16_l3"]
    assert all(np.array_equal(u, v) for u, v in zip(fr.extract(*a[:4]), fr.extract(*b[:4])))
    kp, _ = fr.extract(*fc.extract_cases()["gray_u16_l3"][0:4])
    assert np.bincount(kp[:, 2]).tolist() == [100, 50, 25]      # the per-level budget cuts


def test_score_frames_are_not_vacuous():
    for h, w in fc.score_shapes(ft.TILE_H, ft.TILE_W)[2:]:
        assert np.count_nonzero(fr.score_plane(fc.checkerboard(h, w))[0]) > 0
        assert np.count_nonzero(fr.score_plane(fc.random_gray(h, w, 5))[0]) > 0
        assert np.count_nonzero(fr.score_plane(np.full((h, w), 255, np.uint8))[0]) == 0
    raw = fr.raw_score(fc.checkerboard(48, 128))
    s = fr.score_plane(fc.checkerboard(48, 128))[0]
    assert np.count_nonzero(raw) > np.count_nonzero(s) > 0      # ties everywhere: the suppression decides
    one = fc.random_gray(33, 33, 1)
    one[16, 16], one[13, 16] = 255, 0
    assert fr.raw_score(one)[16, 16] >= 0 and np.count_nonzero(fr.raw_score(one)) <= 1


@pytest.mark.parametrize("name, kind, n, k, seed", fc.RANSAC_CASES, ids=[c[0] for c in fc.RANSAC_CASES])
def test_ransac_cases_meet_what_the_gpu_test_relies_on(name, kind, n, k, seed):
    src, dst, samples = fc.ransac_case(kind, n, k, seed)
    m = 4 if kind == fr.HOMOGRAPHY else 2
    assert samples.shape == (k, m) and samples.min() >= 0 and samples.max() < n
    assert all(len(set(r)) == m for r in samples.tolist())
    counts, models = fr.ransac(src, dst, samples, kind, fc.RANSAC_THR)
    assert counts.max() >= m and (counts >= m).all()            # every sample of these tables is a valid hypothesis
    if n >= 63:
        assert counts.max() >= 0.4 * n                          # and the best finds the planted model
    t2 = fc.RANSAC_THR ** 2
    for i in np.unique(samples, axis=0, return_index=True)[1]:
        r = fr.residuals2(models[i], src, dst, kind)
        assert not (np.abs(r - t2) <= 1e-6).any()               # no residual a rounding could move across the radius
    if kind == fr.HOMOGRAPHY:
        assert fc.system_conds(src, dst, np.unique(samples, axis=0)).max() <= fc.COND_CAP


def test_degenerate_samples_count_minus_one():
    for kind, want in ((fr.SIMILARITY, [True, False, True]), (fr.HOMOGRAPHY, [True, False, True])):
        src, dst, samples = fc.degenerate_case(kind)
        counts, models = fr.ransac(src, dst, samples, kind, fc.RANSAC_THR)
        assert (counts == -1).tolist() == want
        assert not models[counts == -1].any() and models[counts >= 0].any()


def test_sample_table_is_explicit_and_distinct():
    t = fr.sample_table(5, 50, 4, seed=3)
    assert t.dtype == np.int32 and all(len(set(r)) == 4 for r in t.tolist()) and t.max() < 5
    assert np.array_equal(t, fr.sample_table(5, 50, 4, seed=3)) and not np.array_equal(t, fr.sample_table(5, 50, 4, seed=4))
    assert fr.sample_table(1000, 1, 2, seed=0).tolist() == [[16294208416658607535 % 1000, 7960286522194355700 % 1000]]
    with pytest.raises(ValueError):
        fr.sample_table(3, 1, 4)
    for n, k, m, seed in ((77, 40, 4, 9), (5, 300, 4, 1), (2, 70, 2, 2 ** 64 - 3), (1000, 2000, 2, 0)):    # many redraws; a seed that wraps
        assert np.array_equal(ft.sample_table(n, k, m, seed), fr.sample_table(n, k, m, seed)), (n, k, m, seed)


# ------------------------------------------------------------------------------------------------ refit
def test_refit_recovers_exact_models():
    rng = np.random.default_rng(2)
    src = rng.uniform(0.0, 640.0, (40, 2))
    ms = fc.similarity(4.0, 1.05, 12.5, -7.25, 480, 640)
    mh = ms.copy()
    mh[2, 0], mh[2, 1] = 5e-5, -4e-5
    for mod in (fr, ft):
        p = np.concatenate([src, np.ones((40, 1))], axis=1) @ ms.T
        assert np.abs(mod.fit_similarity(src, p[:, :2]) - ms[:2]).max() <= 1e-9
        p = np.concatenate([src, np.ones((40, 1))], axis=1) @ mh.T
        h = mod.fit_homography(src, p[:, :2] / p[:, 2:])
        assert h[2, 2] == 1.0 and np.abs(h - mh).max() <= 1e-9
    m, mask = fr.find_transform(src, (np.concatenate([src, np.ones((40, 1))], axis=1) @ ms.T)[:, :2], fr.SIMILARITY, 3.0, 16)
    assert m.shape == (2, 3) and mask.shape == (40, 1) and mask.dtype == np.uint8 and mask.all()
    assert fr.find_transform(src[:1], src[:1], fr.SIMILARITY) == (None, None)
    assert np.array_equal(ft.residuals2(mh.reshape(9), src, src, 1), fr.residuals2(mh.reshape(9), src, src, 1))
    assert np.array_equal(ft.positions(np.array([[3, 5, 2, 9, 1]])), fr.positions(np.array([[3, 5, 2, 9, 1]])))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def scenes():
    return {"similarity": fc.scene_similarity(), "homography": fc.scene_homography(), "defocus": fc.scene_defocus()}


@pytest.mark.parametrize("scene, kind", [("similarity", fr.SIMILARITY), ("homography", fr.HOMOGRAPHY), ("defocus", fr.SIMILARITY)])
@pytest.mark.parametrize("method", ["NORM_HAMMING", "KNN"])
def test_restatement_recovers_the_transform(scenes, scene, kind, method):
    h, w, m_true, mov, ref = scenes[scene]
    n_good, m = fr.estimate(mov, ref, method, 0.75, kind)
    err = fc.corner_error(m, m_true, h, w)
    print(f"{scene} {method}: {n_good} good matches, largest corner error {err:.3f} px")
    assert n_good >= 100
    assert m.shape == ((3, 3) if kind == fr.HOMOGRAPHY else (2, 3))
    assert err <= 1.0


# ------------------------------------------------------------------------------------------------ the product's host side
def test_params_and_option_handling():
    p = ft.FeatureParams()
    assert (p.levels, p.n_features, p.threshold, p.max_keypoints()) == (3, 2000, 20, 3500)
    for kw in ({"levels": 0}, {"levels": 9}, {"n_features": 0}, {"threshold": 255}, {"threshold": -1}, {"levels": 2.0},
               {"n_features": True}):
        with pytest.raises(InvalidOptionError):
            ft.FeatureParams(**kw)
    est = al.resolve_estimator("features")
    assert callable(est) and est.__name__ == "estimate"
    with pytest.raises(InvalidOptionError, match="'features'"):
        al.resolve_estimator("sift-gpu")
    img = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(InvalidOptionError, match="feature estimator"):
        est(img, img, {}, {}, {"align_method": "LMEDS", "transform": "ALIGN_RIGID"})
    with pytest.raises(InvalidOptionError):
        est(img, img, {}, {}, {"transform": "ALIGN_AFFINE"})
    with pytest.raises(InvalidOptionError):
        ft.match(ft.Features(np.zeros((0, 5), np.int32), np.zeros((0, 32), np.uint8)),
                 ft.Features(np.zeros((0, 5), np.int32), np.zeros((0, 32), np.uint8)), "FLANN")
    for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8, 4), np.uint8), np.zeros((0, 8), np.uint8)):
        with pytest.raises(ValueError):
            ft.detect_and_compute(bad)
    assert ft.find_transform(np.zeros((1, 2)), np.zeros((1, 2))) == (None, None)     # too few points: no device call
    empty = ft.Features(np.zeros((0, 5), np.int32), np.zeros((0, 32), np.uint8))
    assert ft.match(empty, empty).shape == (0, 3)
