"""Alone on the GPU: raw_unpack (mi_raw_unpack_device) at 24 MP and 50 MP for 10, 12, 14 and 16-bit samples, stored as strips
(64 rows) and as 256 x 256 tiles, warm, each against a device copy of the OUTPUT's bytes timed in the same run.  The span holds
random bytes: the kernel's work does not depend on the samples.  Each figure is the median over `--rounds` rounds of `--reps`
back-to-back launches that end in a device synchronise.  `--crop`: an ActiveArea with an odd origin (13, 7), so that no window
starts on a byte boundary.
   python tools/unpack_time.py [--reps 20] [--rounds 7] [--crop] [--json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shinestacker_amd import _lib as L, dng  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--crop", action="store_true", help="crop from (13, 7): windows off the byte boundary")
ap.add_argument("--json", action="store_true", help="print one JSON line per frame size as well")
a = ap.parse_args()

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


rng = np.random.default_rng(3)
for H, W in ((4000, 6000), (5792, 8688)):
    cy, cx = (13, 7) if a.crop else (0, 0)
    h, w = H - cy, W - cx
    ob = h * w * 2
    out, src = L.DeviceBuffer(ob), L.DeviceBuffer(ob)
    res = {}
    try:
        res["copy of the output"] = median_us(lambda: L.check(lib.mi_memcpy_d2d_async(0, None, out.ptr, src.ptr, ob)))
        for bits in (10, 12, 14, 16):
            for kind, (sh, sw) in (("strips", (64, W)), ("tiles", (256, 256))):
                nsy, nsx = -(-H // sh), -(-W // sw)
                rowb = (sw * bits + 7) // 8
                seg = sh * rowb                                         # (the last strip is stored whole here: a little slack)
                offsets = (np.arange(nsy * nsx, dtype=np.uint64) * seg).astype(np.uint32)
                lay = dng.RawLayout(bits, False, H, W, kind == "tiles", sh, sw, offsets, cy, cx, h, w, shift=16 - bits)
                nb = nsy * nsx * seg
                span = L.DeviceBuffer(nb + offsets.nbytes + 256)
                try:
                    span.upload(rng.integers(0, 256, size=nb, dtype=np.uint8))
                    at = (nb + 255) & ~255
                    span.upload(offsets, at)
                    res[f"{bits}-bit {kind}"] = median_us(lambda: dng.unpack_device(lay, span.ptr, nb, span.ptr + at, None, out.ptr)) + (nb,)
                finally:
                    span.free()
        copy = res["copy of the output"][0]
        print(f"{H} x {W} ({H * W / 1e6:.1f} MP){' cropped from (13, 7)' if a.crop else ''}, {a.rounds} rounds of {a.reps} launches: "
              f"median (min .. max) us", flush=True)
        for name, r in res.items():
            moved = 2 * ob if len(r) == 3 else r[3] + ob
            print(f"  {name:20s} {r[0]:9.1f} ({r[1]:9.1f} .. {r[2]:9.1f})   x copy {r[0] / copy:5.2f}   {moved / r[0] / 1e6:5.2f} TB/s "
                  f"(read + written)", flush=True)
        if a.json:
            print(json.dumps({"height": H, "width": W, "crop": [cy, cx], "reps": a.reps, "rounds": a.rounds,
                              "median_us": {k: round(v[0], 1) for k, v in res.items()}}), flush=True)
    finally:
        out.free()
        src.free()
