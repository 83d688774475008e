"""Alone on the GPU: the feature estimator's stages, warm, against two yardsticks timed in the same run -- a device copy of
the frame, and `ecc_estimator` on the same pair.  It reports times only; it is no gate.
   extract        mi_feat_extract_device on a 6 MP uint8 BGR frame resident in HBM (grey, 3 levels, score, select, describe;
                  the call waits: the cut and the sort of each level are host work), and its grey and score kernels alone
   match          mi_feat_match_device, 2000 x 2000 descriptors
   ransac         mi_feat_ransac_device, 2000 hypotheses x 1000 matches, both models
   estimate       feature_estimator on one 6 MP pair from host memory (uploads included), and ecc_estimator on the same pair
   resident       both frames in HBM.  The per-pair entry points: mi_feat_extract_device on the moving frame (and on both
                  frames), features.match and features.find_transform on what it returns.  The handle: FeatureAligner's
                  estimate_batch (refit included) per frame at batch 1 and at batch 16, with the host waits and kernel launches
                  per call from its stats
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

# ---- both frames resident: the per-pair entry points against the handle
BATCH = 16
pair = L.DeviceBuffer((BATCH + 1) * fb)
handle = None
calls = {}
try:
    pair.upload(ref)
    for i in range(BATCH):
        pair.upload(mov, (i + 1) * fb)
    movs = [pair.ptr + (i + 1) * fb for i in range(BATCH)]

    def extract(ptr):
        L.check(lib.mi_feat_extract_device(0, None, ptr, H, W, 3, L.MI_U8, p.levels, p.n_features, p.threshold, table.ctypes.data, cap,
                                           kp.ctypes.data, desc.ctypes.data, C.byref(n)))
        return ft.Features(kp[:n.value].copy(), desc[:n.value].copy())

    f_ref = extract(pair.ptr)

    def per_pair(both):
        f1 = extract(pair.ptr) if both else f_ref
        f0 = extract(movs[0])
        good = ft.match(f0, f1, cfg[1]["match_method"], cfg[1]["threshold"])
        got["per pair, resident"] = (len(good), ft.find_transform(ft.positions(f0.kp)[good[:, 0]], ft.positions(f1.kp)[good[:, 1]],
                                                                  "ALIGN_RIGID", 3.0, 2000)[0])

    few = max(1, a.reps // 5)
    res["resident pair: extract x 2 + match + RANSAC"] = median_us(lambda: per_pair(True), reps=few)
    res["resident pair: extract x 1 + match + RANSAC"] = median_us(lambda: per_pair(False), reps=few)
    handle = ft.FeatureAligner(H, W, np.uint8, p, max_batch=BATCH)
    handle.set_reference(pair.ptr)

    def batch(k):
        got[f"handle, batch {k}"] = handle.estimate_batch(movs[:k], cfg[1], cfg[2])[0][:2]

    for k in (1, BATCH):
        w0, l0 = handle.stats()
        batch(k)
        w1, l1 = handle.stats()
        calls[k] = (w1 - w0, l1 - l0)
        med, lo, hi = median_us(lambda: batch(k), reps=few)
        res[f"handle: estimate_batch of {k}, per frame"] = (med / k, lo / k, hi / k)
finally:
    if handle is not None:
        handle.close()
    pair.free()

print(f"uint8 {H} x {W} x 3 ({H * W / 1e6:.1f} MP), {n_kp} keypoints; {a.rounds} rounds of {a.reps} calls: median (min .. max) us")
for name, (med, lo, hi) in res.items():
    print(f"  {name:36s} {med:10.1f} ({lo:10.1f} .. {hi:10.1f})   x copy {med / res['copy of the frame'][0]:8.2f}")
for name, (ng, m) in got.items():
    print(f"  {name}: n_good {ng}, M = {np.round(np.asarray(m), 4).tolist()}   (the scene's shift is (-7, 5))")
for k, (waits, launches) in calls.items():
    print(f"  handle, one estimate_batch of {k}: {waits} host waits, {launches} kernel launches")
if a.json:
    print(json.dumps({"height": H, "width": W, "keypoints": n_kp, "reps": a.reps, "rounds": a.rounds,
                      "median_us": {k: round(v[0], 1) for k, v in res.items()},
                      "handle_calls": {str(k): {"waits": v[0], "launches": v[1]} for k, v in calls.items()}}))
