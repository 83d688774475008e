"""Frames and cases for the resident feature estimator's tests (features.FeatureAligner, mi_feat_aligner_t).  The
specification is tests/features_restatement.py; the scenes come from tests/features_cases.py.  Everything is generated from
seeds: no files.  tests/test_feature_aligner_host.py checks on the CPU that every case does what its name says."""
import numpy as np

import features_cases as fc
import features_restatement as fr

NEED = {fr.SIMILARITY: 3, fr.HOMOGRAPHY: 4}      # good matches below which nothing is fitted
SAMPLE = {fr.SIMILARITY: 2, fr.HOMOGRAPHY: 4}


def spots(h, w, k, step=12, varied=False, base=30):
    """a grey frame with k isolated bright pixels on a grid of `step` from (18, 18) in raster order; `varied`: 40 different
    brightnesses in turn, hence 40 different scores; else every spot scores alike"""
    g = np.full((h, w), base, np.uint8)
    cols = (w - 2 * fc.EDGE_OFF) // step + 1
    i = np.arange(k)
    y, x = fc.EDGE_OFF + step * (i // cols), fc.EDGE_OFF + step * (i % cols)
    assert k == 0 or (y.max() < h - fr.EDGE and x.max() < w - fr.EDGE), "the spots do not fit"
    g[y, x] = (255 - 4 * (i % 40)) if varied else 255
    return g


# name -> (frame, levels, n_features, threshold): what a level's selection has to deal with
def selection_cases():
    scene = fr.gray(fc.scene_similarity()[4])
    return {
        "none": (np.full((64, 80), 77, np.uint8), 1, 8, 20),
        "one": (spots(64, 80, 1), 1, 8, 20),
        "exactly_n": (spots(64, 160, 8, varied=True), 1, 8, 20),
        "n_plus_one": (spots(64, 160, 9, varied=True), 1, 8, 20),
        "one_score_raster": (fc.dots(240, 320), 1, 8, 20),
        "cut_rises": (spots(400, 800, 6000, step=6, varied=True), 1, 8, 20),
        "one_class_overflows": (fc.dots(300, 400, step=4), 1, 8, 20),
        "lds_bound": (fc.dots(800, 800, step=6), 1, 4096, 20),
        "third_level_too_small": (scene[:100, :100], 3, 2000, 20),
        "side_33": (side_33(), 1, 8, 20),
        "scene_l3": (scene, 3, 2000, 20),
        "scene_truncates": (scene, 3, 100, 20),
    }


def side_33():
    g = np.full((33, 33), 10, np.uint8)
    g[16, 16] = 200
    return g


def level_stats(frame, levels, n_features, threshold):
    """per pyramid level of the restatement: (scored, cut, count(score >= cut), kept)"""
    out = []
    for lv, g in enumerate(fr.pyramid(fr.gray(frame), levels)):
        n_level = n_features >> lv
        scored = n_level >= 1 and g.shape[0] >= 2 * fr.EDGE + 1 and g.shape[1] >= 2 * fr.EDGE + 1
        if not scored:
            out.append((False, 0, 0, 0))
            continue
        score, hist = fr.score_plane(g, threshold)
        cut = fr.select_cut(hist, threshold, n_level)
        n_sel = int(hist[cut:].sum())
        out.append((True, cut, n_sel, min(n_sel, n_level)))
    return out


def gray_cases():
    """name -> (frame, subsample, fast)"""
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (38, 54, 3), dtype=np.uint8)
    u16 = rng.integers(0, 65536, (38, 54, 3), dtype=np.uint16)
    odd = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    return {
        "s1_u8": (u8, 1, True), "s1_u16": (u16, 1, True), "s1_area_flag": (u8, 1, False), "s2_fast": (odd, 2, True),
        "s3_fast": (odd, 3, True), "s2_area_u8": (u8, 2, False), "s2_area_u16": (u16, 2, False),
        "s2_area_u16_saturated": (np.full((6, 8, 3), 65535, np.uint16), 2, False),
        "one_channel_u8": (u8[..., 1].copy(), 1, True), "one_channel_u16_area": (u16[..., 2].copy(), 2, False),
        "one_channel_fast3": (odd[..., 0].copy(), 3, True),
    }


def subsample_area2(img):
    """(a + b + c + d + 2) >> 2 of every 2 x 2 block of a frame with even sides, per channel, by hand"""
    v = img.astype(np.uint32)
    return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).astype(img.dtype)


def expected_pair(mov_sub, ref_sub, levels, n_features, threshold, method, ratio, kind, thr, k, seed):
    """the restatement's every stage for one (already sub-sampled) pair"""
    k0, d0 = fr.extract(mov_sub, levels, n_features, threshold)
    k1, d1 = fr.extract(ref_sub, levels, n_features, threshold)
    good = fr.match(k0, d0, k1, d1, method, ratio)
    src, dst = fr.positions(k0)[good[:, 0]], fr.positions(k1)[good[:, 1]]
    out = dict(kp=k0, desc=d0, ref_kp=k1, ref_desc=d1, good=good, src=src, dst=dst, samples=None, counts=None, models=None,
               winner=-1, m=None)
    if len(good) >= NEED[kind]:
        out["samples"] = fr.sample_table(len(good), k, SAMPLE[kind], seed)
        out["counts"], out["models"] = fr.ransac(src, dst, out["samples"], kind, thr)
        win = int(np.argmax(out["counts"]))
        if out["counts"][win] >= SAMPLE[kind]:
            out["winner"] = win
            out["m"] = fr.refit(src, dst, out["counts"], out["models"], kind, thr)[0]
    return out


def blank(h, w):
    return np.full((h, w, 3), 77, np.uint8)


def one_train_pair():
    """(moving, reference): the reference has ONE keypoint on level 0 (a single spot), the moving frame several"""
    return np.dstack([spots(64, 160, 5, varied=True)] * 3), np.dstack([spots(64, 160, 1)] * 3)


def level_in_one_frame_only():
    """(moving, reference) 3-level frames: the reference's level 1 and 2 have no keypoint (isolated level-0 spots vanish in
    the 2 x 2 mean), the moving frame's have"""
    mov = fc.scene_similarity()[3][:160, :200]
    ref = np.dstack([spots(160, 200, 60, varied=True)] * 3)
    return np.ascontiguousarray(mov), ref


def few_match_cases():
    """name -> (moving, reference, n_features on one level, match method, kind, what RANSAC meets).  A frame against itself
    keeps its n best corners and matches each to itself: n good matches, every hypothesis the identity with all n inliers --
    a tie between all of them, which the lowest index wins.  The five collinear spots against one spot give five matches
    whose every 4-point system is singular."""
    scene = fc.scene_similarity()[4]
    mov, ref = one_train_pair()
    return {
        "two_matches": (scene, scene, 2, "NORM_HAMMING", fr.SIMILARITY, "too_few"),
        "three_matches_tie": (scene, scene, 3, "NORM_HAMMING", fr.SIMILARITY, "tie"),
        "n_equals_m": (scene, scene, 4, "NORM_HAMMING", fr.HOMOGRAPHY, "tie"),
        "six_knn_tie": (scene, scene, 6, "KNN", fr.HOMOGRAPHY, "tie"),
        "all_degenerate": (mov, ref, 8, "KNN", fr.HOMOGRAPHY, "no_winner"),
    }


def pipeline_frames(n=6, h=240, w=320, seed=21):
    """n frames of one canvas under known similarities; frame n // 2 is the untouched crop.  -> (frames, true 3 x 3 list)"""
    c = fc.canvas(h, w, seed)
    rng = np.random.default_rng(seed + 1)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    frames, ms = [], []
    for i in range(n):
        d = i - n // 2
        m = fc.similarity(0.8 * d, 1.0 + 0.006 * d, 2.1 * d, -1.3 * d, h, w)
        u = m[0, 0] * xs + m[0, 1] * ys + m[0, 2]
        v = m[1, 0] * xs + m[1, 1] * ys + m[1, 2]
        f = fc.sample(c, u + fc.MARGIN, v + fc.MARGIN)
        frames.append(np.clip(np.rint(f + rng.normal(0.0, 1.5, f.shape)), 0, 255).astype(np.uint8))
        ms.append(m)
    return frames, ms


RETRY_MIN_GOOD = 100      # between what retry_frame yields sub-sampled by 2 (75) and at full size (107); the others: 111 and up


def retry_frame(h=240, w=320, seed=21):
    """a frame of the pipeline canvas that shows only a window of it, the rest flat: sub-sampled by 2 it yields no more than
    RETRY_MIN_GOOD good matches (the default parameters), at full size more"""
    c = fc.canvas(h, w, seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    m = fc.similarity(0.5, 1.004, 1.5, 0.8, h, w)
    f = fc.sample(c, m[0, 0] * xs + m[0, 1] * ys + m[0, 2] + fc.MARGIN, m[1, 0] * xs + m[1, 1] * ys + m[1, 2] + fc.MARGIN)
    out = np.full((h, w, 3), 90, np.uint8)
    out[40:200, 60:260] = np.clip(np.rint(f), 0, 255).astype(np.uint8)[40:200, 60:260]
    return out, m
