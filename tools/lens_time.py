"""Alone on the GPU: the lens remap (mi_lens_remap_device) on a 24 MP uint8 and a 50 MP uint16 frame, warm, for three lenses --
distortion only (one coordinate set), lateral CA only (green copied), both -- against two yardsticks timed in the same run: a
device copy of the frame, and mi_warp_affine_device without the border blur (tools/warp_time.py's method: the same four-tap
gather at 1/32 pixel with one coordinate set).  Each figure is the median over `--rounds` rounds of `--reps` back-to-back
launches that end in a device synchronise.
   python tools/lens_time.py [--reps 20] [--rounds 7] [--json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shinestacker_amd import Lens, _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--json", action="store_true", help="print one JSON line per frame size as well")
a = ap.parse_args()

LENSES = {"distortion": Lens.distortion(-0.12, 0.02),
          "CA": Lens.chromatic(red=(1.0005, -0.0003), blue=(0.9995, 0.0002)),
          "both": Lens(((0.9995, -0.12, 0.02, 0), (1, -0.12, 0.02, 0), (1.0005, -0.12, 0.02, 0)))}
L.require_device()
lib = L.load()


def median_us(run):
    run()
    lib.mi_device_synchronize(0)
    rounds = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            run()
        lib.mi_device_synchronize(0)
        rounds.append((time.perf_counter() - t0) / a.reps * 1e6)
    return float(np.median(rounds)), float(min(rounds)), float(max(rounds))


for dt, (H, W) in ((np.uint8, (4000, 6000)), (np.uint16, (5792, 8688))):
    dt = np.dtype(dt)
    fb = H * W * 3 * dt.itemsize
    src, dst, tmp, mask = L.DeviceBuffer(fb), L.DeviceBuffer(fb), L.DeviceBuffer(fb), L.DeviceBuffer(H * W)
    try:
        L.synth_frames_device(src.ptr, dt.type, H, W, 0, 1, 4)
        code = L.DTYPE_CODE[dt]
        res = {}
        res["copy"] = median_us(lambda: L.check(lib.mi_memcpy_d2d_async(0, None, dst.ptr, src.ptr, fb)))
        bv = (C.c_double * 4)(0, 0, 0, 0)
        cx, cy = (W - 1) / 2, (H - 1) / 2
        for name, (deg, s, tx, ty) in {"warp 0.2 deg": (0.2, 1.001, 5, -3), "warp zoom 0.98": (0, 0.98, 0, 0)}.items():
            t = np.deg2rad(deg)
            ca, sa = s * np.cos(t), s * np.sin(t)
            M = (C.c_double * 6)(ca, -sa, cx - ca * cx + sa * cy + tx, sa, ca, cy - sa * cx - ca * cy + ty)
            res[name] = median_us(lambda: L.check(lib.mi_warp_affine_device(0, None, src.ptr, dst.ptr, tmp.ptr, mask.ptr, H, W, code, M,
                                                                            1, bv, 21, 50.0)))
        for name, lens in LENSES.items():
            s = lens.struct(H, W)
            res["lens " + name] = median_us(lambda: L.check(lib.mi_lens_remap_device(0, None, src.ptr, dst.ptr, None, H, W, code,
                                                                                      C.byref(s))))
            res["lens " + name + " + mask"] = median_us(lambda: L.check(lib.mi_lens_remap_device(0, None, src.ptr, dst.ptr, mask.ptr, H, W,
                                                                                                 code, C.byref(s))))
        warp = min(res["warp 0.2 deg"][0], res["warp zoom 0.98"][0])
        print(f"{dt.name} {H} x {W} ({H * W / 1e6:.1f} MP), {a.rounds} rounds of {a.reps} launches: median (min .. max) us", flush=True)
        for name, (med, lo, hi) in res.items():
            print(f"  {name:24s} {med:9.1f} ({lo:9.1f} .. {hi:9.1f})   x copy {med / res['copy'][0]:5.2f}   x warp {med / warp:5.2f}   "
                  f"{2 * fb / med / 1e6:5.2f} TB/s (src + dst)", flush=True)
        if a.json:
            print(json.dumps({"dtype": dt.name, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds,
                              "median_us": {k: round(v[0], 1) for k, v in res.items()}}), flush=True)
    finally:
        for b in (src, dst, tmp, mask):
            b.free()
