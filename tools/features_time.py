"""Alone on the GPU: the feature estimator's stages, warm, against two yardsticks timed in the same run -- a device copy of
the frame, and `ecc_estimator` on the same pair.  It reports times only; it is no gate.
   extract        mi_feat_extract_device on a 6 MP uint8 BGR frame resident in HBM (grey, 3 levels, score, select, describe;
                  the call waits: the cut and the sort of each level are host work), and its grey and score kernels alone
   match          mi_feat_match_device, 2000 x 2000 descriptors
   ransac         mi_feat_ransac_device, 2000 hypotheses x 1000 matches, both models
   estimate       feature_estimator on one 6 MP pair from host memory (uploads included), and ecc_estimator on the same pair
Each figure is the median over `--rounds` rounds of `--reps` back-to-back calls that end in a device synchronise.
   python tools/features_time.py [--reps 10] [--rounds 5] [--json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shinestacker_amd import _lib as L  # noqa: E402
from shinestacker_amd import align as al  # noqa: E402
from shinestacker_amd import features as ft  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", action="store_true", help="print one JSON line as well")
a = ap.parse_args()

L.require_device()
lib = L.load()
H, W = 2000, 3000


def median_us(run, reps=None):
    reps = reps or a.reps
    run()
    lib.mi_device_synchronize(0)
    rounds = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            run()
        lib.mi_device_synchronize(0)
        rounds.append((time.perf_counter() - t0) / reps * 1e6)
    return float(np.median(rounds)), float(min(rounds)), float(max(rounds))


def scene(h, w, seed):
    """random overlapping rectangles with 1.5 grey levels of noise: (moving, reference), the moving frame maps onto the reference by a shift of (-7, 5)"""
    rng = np.random.default_rng(seed)
    c = np.full((h + 32, w + 32, 3), 90, np.uint8)
    for _ in range(h * w // 500):
        rh, rw = rng.integers(8, 56, 2)
        y, x = rng.integers(0, h + 24), rng.integers(0, w + 24)
        c[y:y + rh, x:x + rw] = rng.integers(20, 236, 3)

    def noisy(f):
        return np.clip(f + np.rint(rng.normal(0.0, 1.5, f.shape)), 0, 255).astype(np.uint8)
    return noisy(c[21:21 + h, 9:9 + w].astype(np.float32)), noisy(c[16:16 + h, 16:16 + w].astype(np.float32))


mov, ref = scene(H, W, 1)
fb = ref.nbytes
res = {}
frame, copy, gray, score, hist = (L.DeviceBuffer(n) for n in (fb, fb, H * W, H * W, 1024))
try:
    frame.upload(ref)
    res["copy of the frame"] = median_us(lambda: L.check(lib.mi_memcpy_d2d_async(0, None, copy.ptr, frame.ptr, fb)))
    res["gray"] = median_us(lambda: L.check(lib.mi_feat_gray_device(0, None, frame.ptr, H, W, 3, L.MI_U8, gray.ptr)))
    res["score + suppression + histogram"] = median_us(
        lambda: L.check(lib.mi_feat_score_device(0, None, gray.ptr, H, W, 20, score.ptr, hist.ptr)))
    p = ft.FeatureParams()
    cap = p.max_keypoints()
    kp, desc, n = np.empty((cap, 5), np.int32), np.empty((cap, 32), np.uint8), C.c_int(0)
    table = ft.pattern()
    res["extract (frame in HBM)"] = median_us(lambda: L.check(lib.mi_feat_extract_device(
        0, None, frame.ptr, H, W, 3, L.MI_U8, p.levels, p.n_features, p.threshold, table.ctypes.data, cap, kp.ctypes.data,
        desc.ctypes.data, C.byref(n))))
    n_kp = n.value
finally:
    for b in (frame, copy, gray, score, hist):
        b.free()

rng = np.random.default_rng(2)
d0 = rng.integers(0, 256, (2000, 32), dtype=np.uint8)
d1 = rng.integers(0, 256, (2000, 32), dtype=np.uint8)
src = rng.uniform(0.0, 3000.0, (1000, 2))
dst = src * 1.01 + rng.normal(0.0, 0.3, src.shape)
bufs = [L.DeviceBuffer(n) for n in (d0.nbytes, d1.nbytes, 2000 * 12, src.nbytes, dst.nbytes, 2000 * 16, 2000 * 4, 2000 * 72)]
try:
    q, t, out, s, d, sam, cnt, mod = bufs
    q.upload(d0)
    t.upload(d1)
    s.upload(src)
    d.upload(dst)
    res["match 2000 x 2000"] = median_us(lambda: L.check(lib.mi_feat_match_device(0, None, q.ptr, 2000, t.ptr, 2000, out.ptr)))
    for name, kind, m in (("similarity", ft.SIMILARITY, 2), ("homography", ft.HOMOGRAPHY, 4)):
        sam.upload(ft.sample_table(1000, 2000, m, 0))
        res[f"ransac 2000 x 1000, {name}"] = median_us(lambda: L.check(lib.mi_feat_ransac_device(
            0, None, s.ptr, d.ptr, 1000, sam.ptr, 2000, kind, 3.0, cnt.ptr, mod.ptr)))
finally:
    for b in bufs:
        b.free()

cfg = ({}, {"match_method": "KNN", "threshold": 0.75}, {"transform": "ALIGN_RIGID", "align_method": "RANSAC", "rans_threshold": 3.0,
                                                          "max_iters": 2000})
feat, ecc = ft.feature_estimator(), al.ecc_estimator()
got = {}


def run(name, est):
    got[name] = est(mov, ref, *cfg)


res["estimate, features (host frames)"] = median_us(lambda: run("features", feat), reps=max(1, a.reps // 5))
res["estimate, ECC (host frames)"] = median_us(lambda: run("ecc", ecc), reps=max(1, a.reps // 5))

print(f"uint8 {H} x {W} x 3 ({H * W / 1e6:.1f} MP), {n_kp} keypoints; {a.rounds} rounds of {a.reps} calls: median (min .. max) us")
for name, (med, lo, hi) in res.items():
    print(f"  {name:36s} {med:10.1f} ({lo:10.1f} .. {hi:10.1f})   x copy {med / res['copy of the frame'][0]:8.2f}")
for name, (ng, m) in got.items():
    print(f"  {name}: n_good {ng}, M = {np.round(np.asarray(m), 4).tolist()}   (the scene's shift is (-7, 5))")
if a.json:
    print(json.dumps({"height": H, "width": W, "keypoints": n_kp, "reps": a.reps, "rounds": a.rounds,
                      "median_us": {k: round(v[0], 1) for k, v in res.items()}}))
