"""The feature estimator on the MI355X: `estimator="features"` (csrc/kernels_features.hpp, csrc/features_host.hpp).

The reference's default alignment recipe detects keypoints, describes them, matches the descriptors and fits a similarity or
a homography with RANSAC (align.py:48-151), all through OpenCV.  This is that recipe as an algorithm of our own of the ORB
family -- it is NOT OpenCV's ORB and is pinned against nothing but tests/features_restatement.py, which is its specification:

    grey (integer) -> `levels` factor-2 levels -> FAST-9 score + 3 x 3 suppression -> the best n_features >> level per level
    -> 32-bin intensity-centroid orientation -> 256 rotated 5 x 5 box-sum tests -> Hamming match per level (cross-check or
    ratio test) -> RANSAC over a seeded sample table, every hypothesis evaluated -> least-squares refit in NumPy

Everything up to the matcher is integer and exact; RANSAC is float64 with one rounding per operation on the device, the
refit float64 NumPy on the host.  There is no CPU path for the device stages: without a GPU they raise DeviceError.
`FeatureParams`, `pattern`, `positions`, `sample_table` and the refit are host NumPy.

`feature_estimator` works on a pair of host frames.  `FeatureAligner` is the same estimator on frames resident in device memory:
one handle, the reference frame's features extracted once, a batch of moving frames per call (mi_feat_aligner_t).
"""
import logging
from collections import namedtuple

import numpy as np

from . import _lib
from .defaults import constants
from .errors import InvalidOptionError

EDGE = 16                          # feat::EDGE of csrc/kernels_features.hpp
TILE_H, TILE_W = 16, 64            # feat::TILE_H / TILE_W, the score kernel's tile
MATCH_NT, MATCH_CHUNK = 64, 256    # feat::MATCH_NT / MATCH_CHUNK, the matcher's block and LDS chunk
BINS, N_TESTS = 32, 256
MAX_LEVELS, MAX_FEATURES = 8, 1 << 16
SIMILARITY, HOMOGRAPHY = 0, 1      # MI_FEAT_SIMILARITY / MI_FEAT_HOMOGRAPHY
NO_SECOND = 0xFFFF

Features = namedtuple("Features", "kp desc")
Features.__doc__ = "kp: N x 5 int32 (x, y, level, score, bin), levels in order; desc: N x 32 uint8"


class FeatureParams:
    """levels      pyramid levels, 1 .. 8 (level l + 1 is the 2 x 2 mean of level l)
    n_features  keypoints kept on level 0; level l keeps n_features >> l
    threshold   a pixel is a corner when its FAST-9 score exceeds it, 0 .. 254"""

    def __init__(self, levels=3, n_features=2000, threshold=20):
        for name, v, lo, hi in (("levels", levels, 1, MAX_LEVELS), ("n_features", n_features, 1, MAX_FEATURES),
                                ("threshold", threshold, 0, 254)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise InvalidOptionError(name, v, f"an integer in [{lo}, {hi}] is expected")
        self.levels, self.n_features, self.threshold = int(levels), int(n_features), int(threshold)

    def max_keypoints(self):
        return sum(self.n_features >> lv for lv in range(self.levels))

    def __repr__(self):
        return f"FeatureParams(levels={self.levels}, n_features={self.n_features}, threshold={self.threshold})"


_PATTERN = None
_MASK64 = (1 << 64) - 1
_GAMMA = np.uint64(0x9E3779B97F4A7C15)


def pattern():
    """The 32 x 256 x 4 int8 test table (xa, ya, xb, yb), built once.  The base tests come from an explicit 64-bit linear
    congruential generator (seed 12345), so that no library's random stream is involved: each coordinate is
    clip(rint(5 g), -9, 9), g = the sum of 12 uniform draws (s >> 33) / 2^31 minus 6; a test whose points coincide is drawn
    again.  Row k holds the base tests rotated by 2 pi k / 32 and rounded: the largest offset is 13."""
    global _PATTERN
    if _PATTERN is None:
        state, mask = 12345, (1 << 64) - 1
        base = []
        while len(base) < N_TESTS:
            t = []
            for _ in range(4):
                acc = 0.0
                for _ in range(12):
                    state = (state * 6364136223846793005 + 1442695040888963407) & mask
                    acc += (state >> 33) / 2147483648.0
                t.append(min(max(float(np.rint(5.0 * (acc - 6.0))), -9.0), 9.0))
            if (t[0], t[1]) != (t[2], t[3]):
                base.append(t)
        base = np.array(base, np.float64)
        table = np.empty((BINS, N_TESTS, 4), np.int8)
        for k in range(BINS):
            c, s = np.cos(2.0 * np.pi * k / BINS), np.sin(2.0 * np.pi * k / BINS)
            for o in (0, 2):
                table[k, :, o] = np.rint(base[:, o] * c - base[:, o + 1] * s)
                table[k, :, o + 1] = np.rint(base[:, o] * s + base[:, o + 1] * c)
        table.setflags(write=False)
        _PATTERN = table
    return _PATTERN


def _frame(img):
    a = np.asarray(img)
    if a.dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise ValueError(f"a uint8 or uint16 frame is expected, got {a.dtype}")
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"an H x W or H x W x 3 (BGR) frame is expected, got shape {a.shape}")
    return np.ascontiguousarray(a)


def gray(img, device=0):
    """the 8-bit grey plane the estimator works on (mi_feat_gray)"""
    a = _frame(img)
    h, w = a.shape[:2]
    _lib.require_device()
    out = np.empty((h, w), np.uint8)
    _lib.check(_lib.load().mi_feat_gray(device, a.ctypes.data, h, w, 1 if a.ndim == 2 else 3, _lib.DTYPE_CODE[a.dtype],
                                        out.ctypes.data))
    return out


def score(gray_plane, threshold=20, device=0):
    """H x W uint8 grey -> (the uint8 score plane after suppression, its 256-bin uint32 histogram) (mi_feat_score)"""
    g = np.ascontiguousarray(gray_plane)
    if g.dtype != np.uint8 or g.ndim != 2 or g.size == 0:
        raise ValueError("an H x W uint8 grey plane is expected")
    _lib.require_device()
    out = np.empty_like(g)
    hist = np.empty(256, np.uint32)
    _lib.check(_lib.load().mi_feat_score(device, g.ctypes.data, g.shape[0], g.shape[1], int(threshold), out.ctypes.data,
                                         hist.ctypes.data))
    return out, hist


def detect_and_compute(img, params=None, device=0):
    """keypoints and descriptors of one frame (H x W x 3 BGR or H x W; uint8 or uint16; anything else is a ValueError)"""
    params = params or FeatureParams()
    a = _frame(img)
    h, w = a.shape[:2]
    _lib.require_device()
    cap = params.max_keypoints()
    kp = np.empty((cap, 5), np.int32)
    desc = np.empty((cap, 32), np.uint8)
    n = _lib.C.c_int(0)
    table = pattern()
    _lib.check(_lib.load().mi_feat_extract(device, a.ctypes.data, h, w, 1 if a.ndim == 2 else 3, _lib.DTYPE_CODE[a.dtype],
                                           params.levels, params.n_features, params.threshold, table.ctypes.data, cap,
                                           kp.ctypes.data, desc.ctypes.data, _lib.C.byref(n)))
    return Features(kp[:n.value].copy(), desc[:n.value].copy())


def positions(kp):
    """level-0 positions, N x 2 float64: x 2^l + (2^l - 1) / 2"""
    kp = np.asarray(kp).reshape(-1, 5)
    f = np.exp2(kp[:, 2].astype(np.float64))
    return np.stack([kp[:, 0] * f + (f - 1.0) / 2.0, kp[:, 1] * f + (f - 1.0) / 2.0], axis=1)


def match_descriptors(query, train, device=0):
    """nq x 3 int32 per query descriptor: the nearest train descriptor (lowest index on ties), its Hamming distance, and the
    smallest distance among all other train descriptors (0xFFFF when there is none) (mi_feat_match)"""
    q, t = np.ascontiguousarray(query), np.ascontiguousarray(train)
    for a in (q, t):
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != 32 or a.shape[0] < 1:
            raise ValueError("N x 32 uint8 descriptors, N >= 1, are expected")
    _lib.require_device()
    out = np.empty((q.shape[0], 3), np.int32)
    _lib.check(_lib.load().mi_feat_match(device, q.ctypes.data, q.shape[0], t.ctypes.data, t.shape[0], out.ctypes.data))
    return out


def match(f0, f1, method=constants.MATCHING_KNN, threshold=0.75, device=0):
    """The good matches of two frames' features, M x 3 int32 (index into f0, index into f1, distance).  A keypoint matches
    only keypoints of its own level.  NORM_HAMMING: the pairs that are each other's nearest (cross-check), sorted by distance
    then query index.  KNN: the reference's ratio test d1 < threshold * d2, in query order."""
    if method not in (constants.MATCHING_KNN, constants.MATCHING_NORM_HAMMING):
        raise InvalidOptionError('match_method', method,
                                 f". Valid options are: {constants.MATCHING_KNN}, {constants.MATCHING_NORM_HAMMING}")
    kp0, kp1 = np.asarray(f0.kp).reshape(-1, 5), np.asarray(f1.kp).reshape(-1, 5)
    out = []
    for lv in sorted(set(kp0[:, 2].tolist()) & set(kp1[:, 2].tolist())):
        i0, i1 = np.nonzero(kp0[:, 2] == lv)[0], np.nonzero(kp1[:, 2] == lv)[0]
        fwd = match_descriptors(f0.desc[i0], f1.desc[i1], device)
        if method == constants.MATCHING_NORM_HAMMING:
            back = match_descriptors(f1.desc[i1], f0.desc[i0], device)
            good = back[fwd[:, 0], 0] == np.arange(len(i0))
        else:
            good = fwd[:, 1].astype(np.float64) < np.float64(threshold) * fwd[:, 2].astype(np.float64)
        out.append(np.stack([i0[good], i1[fwd[good, 0]], fwd[good, 1]], axis=1))
    m = np.concatenate(out).astype(np.int32) if out else np.zeros((0, 3), np.int32)
    if method == constants.MATCHING_NORM_HAMMING:
        return m[np.lexsort((m[:, 0], m[:, 2]))]
    return m[np.argsort(m[:, 0], kind="stable")]


def sample_table(n, k, m, seed=0):
    """K x m int32 match indices for RANSAC: every row m distinct indices below n, drawn as splitmix64(seed) % n, a repeat
    within a row drawn again"""
    n, k, m = int(n), int(k), int(m)
    if n < m:
        raise ValueError("fewer matches than a sample needs")
    out = np.empty((k, m), np.int32)
    drawn, pos, vals = 0, 0, []
    for r in range(k):
        row = []
        while len(row) < m:
            if pos == len(vals):      # the next stretch of the stream at once: splitmix64 is a counter run through a mixer
                count = max(64, (k - r) * m)
                z = (np.uint64(int(seed) & _MASK64) + np.arange(drawn + 1, drawn + count + 1, dtype=np.uint64) * _GAMMA)
                z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
                z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
                vals, pos, drawn = ((z ^ (z >> np.uint64(31))) % np.uint64(n)).tolist(), 0, drawn + count
            v = vals[pos]
            pos += 1
            if v not in row:
                row.append(v)
        out[r] = row
    return out


def ransac(src, dst, samples, kind, thr, device=0):
    """every hypothesis of `samples` evaluated on the device (mi_feat_ransac): (counts K int32, models K x 9 float64)"""
    src = np.ascontiguousarray(np.asarray(src, np.float64).reshape(-1, 2))
    dst = np.ascontiguousarray(np.asarray(dst, np.float64).reshape(-1, 2))
    samples = np.ascontiguousarray(samples, np.int32)
    m = 4 if kind == HOMOGRAPHY else 2
    if samples.ndim != 2 or samples.shape[1] != m or len(src) != len(dst):
        raise ValueError(f"K x {m} samples and two N x 2 point sets are expected")
    _lib.require_device()
    k = samples.shape[0]
    counts = np.empty(k, np.int32)
    models = np.empty((k, 9), np.float64)
    _lib.check(_lib.load().mi_feat_ransac(device, src.ctypes.data, dst.ctypes.data, len(src), samples.ctypes.data, k, int(kind),
                                          float(thr), counts.ctypes.data, models.ctypes.data))
    return counts, models


def residuals2(model, src, dst, kind):
    """the squared residual of every match under a 3 x 3 model given as 9 values, in the device's order of operations; inf
    where a homography's denominator is below 1e-12 in magnitude"""
    x, y, u, v = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    m = model
    if kind == SIMILARITY:
        ex = ((m[0] * x + m[1] * y) + m[2]) - u
        ey = ((m[3] * x + m[4] * y) + m[5]) - v
        return ex * ex + ey * ey
    w = (m[6] * x + m[7] * y) + 1.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ex = ((m[0] * x + m[1] * y) + m[2]) / w - u
        ey = ((m[3] * x + m[4] * y) + m[5]) / w - v
        r = ex * ex + ey * ey
    return np.where(np.abs(w) < 1e-12, np.inf, r)


def fit_similarity(src, dst):
    """the 4-parameter linear least squares over the matches: 2 x 3"""
    n = len(src)
    a = np.zeros((2 * n, 4))
    a[0::2] = np.stack([src[:, 0], -src[:, 1], np.ones(n), np.zeros(n)], axis=1)
    a[1::2] = np.stack([src[:, 1], src[:, 0], np.zeros(n), np.ones(n)], axis=1)
    p = np.linalg.lstsq(a, dst.reshape(-1), rcond=None)[0]
    return np.array([[p[0], -p[1], p[2]], [p[1], p[0], p[3]]])


def _hartley(p):
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    s = np.sqrt(2.0) / d if d > 0 else 1.0
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def fit_homography(src, dst):
    """Hartley-normalised DLT through the SVD over the matches: 3 x 3 with h22 = 1"""
    ts, td = _hartley(src), _hartley(dst)
    p = src * ts[0, 0] + ts[:2, 2]
    q = dst * td[0, 0] + td[:2, 2]
    n = len(src)
    a = np.zeros((2 * n, 9))
    a[0::2, 0:2], a[0::2, 2] = p, 1.0
    a[0::2, 6:8], a[0::2, 8] = -q[:, :1] * p, -q[:, 0]
    a[1::2, 3:5], a[1::2, 5] = p, 1.0
    a[1::2, 6:8], a[1::2, 8] = -q[:, 1:] * p, -q[:, 1]
    h = np.linalg.svd(a)[2][-1].reshape(3, 3)
    h = np.linalg.inv(td) @ h @ ts
    return h / h[2, 2]


def _kind(transform):
    if transform == constants.ALIGN_RIGID:
        return SIMILARITY
    if transform == constants.ALIGN_HOMOGRAPHY:
        return HOMOGRAPHY
    raise InvalidOptionError("transform", transform)


def find_transform(src_pts, dst_pts, transform=constants.DEFAULT_TRANSFORM, rans_threshold=3.0, max_iters=2000, seed=0, device=0):
    """RANSAC on the device, refit on the host: (M, mask) shaped as cv2 returns them -- 2 x 3 for ALIGN_RIGID, 3 x 3 with
    h22 = 1 for ALIGN_HOMOGRAPHY, mask N x 1 uint8 -- or (None, None) when nothing can be fitted.  All `max_iters`
    hypotheses are evaluated (they run in parallel: there is no adaptive stop); the winner is the largest count, the lowest
    index on ties.  Similarity: linear least squares over the winner's inliers.  Homography: normalised DLT over them, the
    inliers selected once more with the refit model, and a second fit."""
    kind = _kind(transform)
    src, dst = np.asarray(src_pts, np.float64).reshape(-1, 2), np.asarray(dst_pts, np.float64).reshape(-1, 2)
    if len(src) != len(dst):
        raise ValueError("as many source as destination points are expected")
    if not (isinstance(max_iters, (int, np.integer)) and max_iters >= 1):
        raise InvalidOptionError("max_iters", max_iters, "an integer >= 1 is expected")
    m = 4 if kind == HOMOGRAPHY else 2
    if len(src) < m:
        return None, None
    counts, models = ransac(src, dst, sample_table(len(src), max_iters, m, seed), kind, rans_threshold, device)
    win = int(np.argmax(counts))
    if counts[win] < m:
        return None, None
    t2 = np.float64(rans_threshold) * np.float64(rans_threshold)
    return _refit(src, dst, residuals2(models[win], src, dst, kind) <= t2, kind, t2)


def _refit(src, dst, inl, kind, t2):
    """the least-squares fit over the winning hypothesis' inliers `inl`: (M, mask) as find_transform returns them"""
    if kind == SIMILARITY:
        return fit_similarity(src[inl], dst[inl]), inl.astype(np.uint8).reshape(-1, 1)
    h = fit_homography(src[inl], dst[inl])
    again = residuals2(h.reshape(9), src, dst, kind) <= t2
    if again.sum() >= 4:
        inl = again
        h = fit_homography(src[inl], dst[inl])
    return h, inl.astype(np.uint8).reshape(-1, 1)


_logged = False


def feature_estimator(params=None, device=0, seed=0):
    """An estimator for `align_images` / `AlignFrames` (`estimator="features"`): (img_0_sub, img_1_sub, feature_config,
    matching_config, alignment_config) -> (n_good, M), n_good the number of good matches before RANSAC as in the reference.
    Honoured: match_method, threshold, transform, rans_threshold, max_iters.  align_method='LMEDS' is refused.  detector and
    descriptor are ignored -- this estimator has one of each -- and what runs is logged once."""
    params = params or FeatureParams()

    def estimate(img_0_sub, img_1_sub, feature_config, matching_config, alignment_config):
        global _logged
        feature_config, matching_config, alignment_config = feature_config or {}, matching_config or {}, alignment_config or {}
        method = alignment_config.get('align_method', constants.ALIGN_RANSAC)
        if method != constants.ALIGN_RANSAC:
            raise InvalidOptionError('align_method', method, ": the feature estimator (estimator='features') fits with RANSAC only")
        transform = alignment_config.get('transform', constants.DEFAULT_TRANSFORM)
        kind = _kind(transform)
        if not _logged:
            _logged = True
            logging.getLogger("shinestacker_amd").info(
                "estimator='features': FAST-9 corners and 256-bit rotated box-sum descriptors on %d pyramid levels run whatever "
                "detector / descriptor is configured (here %s / %s)", params.levels, feature_config.get('detector'),
                feature_config.get('descriptor'))
        f0 = detect_and_compute(img_0_sub, params, device)
        f1 = detect_and_compute(img_1_sub, params, device)
        good = match(f0, f1, matching_config.get('match_method', constants.MATCHING_KNN), matching_config.get('threshold', 0.75),
                     device)
        if len(good) < (4 if kind == HOMOGRAPHY else 3):
            return len(good), None
        m, _ = find_transform(positions(f0.kp)[good[:, 0]], positions(f1.kp)[good[:, 1]], transform,
                              alignment_config.get('rans_threshold', 3.0), alignment_config.get('max_iters', 2000), seed, device)
        return len(good), m
    return estimate


def check_subsampling(height, width, subsample, fast):
    """The handle sub-samples on the device: `fast` for any factor, the area mean for a factor of 2 on even sides.  Every
    other area case goes through float32 arithmetic that is pinned against nothing, and is refused."""
    s = int(subsample)
    if s < 1:
        raise InvalidOptionError("subsample", subsample, "an integer >= 1 is expected")
    if not fast and s > 1 and (s != 2 or height % 2 or width % 2):
        raise InvalidOptionError("subsample", subsample,
                                 f": the resident feature estimator sub-samples by area for subsample=2 on frames of even "
                                 f"height and width only (got subsample={s} on {height} x {width}); set fast_subsampling=True "
                                 "to run this case")
    return s


class FeatureAligner:
    """`feature_estimator` for frames that are resident in device memory (mi_feat_aligner_t, csrc/features_host.hpp): one
    handle holds every buffer for `max_batch` moving frames and the reference frame, whose keypoints and descriptors are
    extracted once (`set_reference`).  `estimate_batch` runs every stage for the whole batch with the frame index in the
    grid -- the cut and the sort of each level on the device -- and the host waits twice per call: for the good-match counts,
    from which the library draws the sample tables, and for the results.  The refit is `find_transform`'s, in NumPy.

    `n_features` is at most 4096 here (the selection sorts a level's candidates in one workgroup's LDS) and `max_iters` at
    most 4096 (the hypothesis buffers are allocated with the handle); `feature_estimator` has neither limit."""

    def __init__(self, height, width, dtype, params=None, subsample=1, fast=True, max_batch=16, device=0, seed=0, channels=3):
        self.params = params or FeatureParams()
        self.height, self.width, self.subsample = int(height), int(width), check_subsampling(height, width, subsample, fast)
        self.fast = bool(fast) or self.subsample == 1
        if self.params.n_features > _lib.FeatureAligner.MAX_FEATURES:
            raise InvalidOptionError("n_features", self.params.n_features,
                                     f": the resident feature estimator keeps at most {_lib.FeatureAligner.MAX_FEATURES} keypoints "
                                     "on level 0 (a level's candidates are sorted in one workgroup's LDS)")
        if isinstance(max_batch, bool) or not isinstance(max_batch, (int, np.integer)) or not 1 <= max_batch <= _lib.FeatureAligner.MAX_BATCH:
            raise InvalidOptionError("max_batch", max_batch, f"an integer in [1, {_lib.FeatureAligner.MAX_BATCH}] is expected")
        self.seed, self.device, self.max_batch = seed, device, int(max_batch)
        self._al = None
        _lib.require_device()
        self._al = _lib.FeatureAligner(height, width, dtype, pattern(), channels=channels, subsample=self.subsample, fast=self.fast,
                                       levels=self.params.levels, n_features=self.params.n_features,
                                       threshold=self.params.threshold, max_batch=self.max_batch, device=device)
        self.shape_sub = self._al.shape

    @staticmethod
    def options(matching_config, alignment_config):
        """(match method code, ratio, kind, transform, rans_threshold, max_iters) of the configuration dictionaries, refused as
        `feature_estimator` refuses them"""
        matching_config, alignment_config = matching_config or {}, alignment_config or {}
        method = alignment_config.get('align_method', constants.ALIGN_RANSAC)
        if method != constants.ALIGN_RANSAC:
            raise InvalidOptionError('align_method', method, ": the feature estimator (estimator='features') fits with RANSAC only")
        transform = alignment_config.get('transform', constants.DEFAULT_TRANSFORM)
        kind = _kind(transform)
        match_method = matching_config.get('match_method', constants.MATCHING_KNN)
        if match_method not in (constants.MATCHING_KNN, constants.MATCHING_NORM_HAMMING):
            raise InvalidOptionError('match_method', match_method,
                                     f". Valid options are: {constants.MATCHING_KNN}, {constants.MATCHING_NORM_HAMMING}")
        max_iters = alignment_config.get('max_iters', 2000)
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or not 1 <= max_iters <= _lib.FeatureAligner.MAX_ITERS:
            raise InvalidOptionError("max_iters", max_iters, f"an integer in [1, {_lib.FeatureAligner.MAX_ITERS}] is expected by the "
                                     "resident feature estimator")
        code = _lib.FEAT_MATCH_KNN if match_method == constants.MATCHING_KNN else _lib.FEAT_MATCH_HAMMING
        return (code, float(matching_config.get('threshold', 0.75)), kind, transform,
                float(alignment_config.get('rans_threshold', 3.0)), int(max_iters))

    def set_reference(self, dev_ptr):
        self._al.set_reference(dev_ptr)

    def estimate_raw(self, dev_ptrs, matching_config=None, alignment_config=None):
        """the library's per-frame results (`_lib.FeatureAligner.estimate_batch`) for the configuration dictionaries"""
        code, ratio, kind, _, thr, max_iters = self.options(matching_config, alignment_config)
        return self._al.estimate_batch(list(dev_ptrs), code, ratio, kind, thr, max_iters, self.seed)

    def estimate_batch(self, dev_ptrs, matching_config=None, alignment_config=None):
        """-> per frame (n_good, M, inlier_fraction): M maps the moving frame onto the reference in full-resolution pixels
        (`align.rescale_transform`), 2 x 3 or 3 x 3, or None with fewer than 3 / 4 good matches or without a model;
        inlier_fraction = the refit's inliers / n_good (0.0 without a model)"""
        from .align import rescale_transform
        _, _, kind, transform, thr, _ = self.options(matching_config, alignment_config)
        t2 = np.float64(thr) * np.float64(thr)
        out = []
        for r in self.estimate_raw(dev_ptrs, matching_config, alignment_config):
            if r["n_good"] < (4 if kind == HOMOGRAPHY else 3) or r["winner"] < 0:
                out.append((r["n_good"], None, 0.0))
                continue
            m, mask = _refit(r["src"], r["dst"], r["mask"].astype(bool), kind, t2)
            if self.subsample > 1:
                m = rescale_transform(m, transform, self.subsample, (self.height, self.width), self.shape_sub)
            out.append((r["n_good"], m, float(mask.sum()) / r["n_good"]))
        return out

    def tap(self, frame_slot, what, level=0):
        return self._al.tap(frame_slot, what, level)

    def stats(self):
        return self._al.stats()

    def close(self):
        if self._al is not None:
            self._al.close()
            self._al = None
