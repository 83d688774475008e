"""Alone on the GPU: mosaic_site_correct (mi_mosaic_site_correct_device, in place) on a resident mosaic of 24 MP uint8 and of
50 MP uint16, with the black deltas only, the gain maps only and both; the maps are 17 x 13 and 257 x 257 nodes per position
(four maps).  Every timing sits beside a device-to-device copy of the same mosaic (read once, written once: the bytes the
pass moves, its tables fit in cache) taken in the same run.

    python tools/sitecorr_time.py [--runs 20] [--small] [--json FILE]

Method, as tools/demosaic_time.py: hipEvents around 5 back-to-back launches, 3 warm-up launches, the median of `--runs`
windows; the whole list is measured twice and the second pass is reported (the first warms clocks and caches).  The kernel
corrects the same mosaic in place over and over: the values settle, the work per launch does not change.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shinestacker_amd import _lib as L  # noqa: E402
from shinestacker_amd import demosaic, dng  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--small", action="store_true", help="a 1 MP rehearsal of the whole script")
ap.add_argument("--json", default=None)
a = ap.parse_args()
L.require_device()
lib = L.load()


def hip_runtime():
    """the HIP runtime the library brought into this process, for its events"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime in this process")


hip = hip_runtime()
for fn in (hip.hipEventCreate, hip.hipEventRecord, hip.hipEventSynchronize, hip.hipEventElapsedTime):
    fn.restype = C.c_int
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def ck(rc, what):
    if rc != 0:
        raise SystemExit(f"{what}: HIP error {rc}")


e0, e1 = C.c_void_p(), C.c_void_p()
ck(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
ck(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
PER, WARM = 5, 3        # launches per timed window (a single launch of ~0.05 ms would measure the events), warm-up launches


def measure(fn):
    for _ in range(WARM):
        fn()
    L.check(lib.mi_device_synchronize(0))
    times = []
    for _ in range(a.runs):
        ck(hip.hipEventRecord(e0, None), "hipEventRecord")
        for _ in range(PER):
            fn()
        ck(hip.hipEventRecord(e1, None), "hipEventRecord")
        ck(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float()
        ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        times.append(ms.value / PER)
    return statistics.median(times)


def gain_maps(mv, mh):
    return [dng.GainMap(np.random.default_rng([mv, mh, p]).uniform(0.8, 1.25, size=(mv, mh)),
                        spacing=(1.0 / (mv - 1), 1.0 / (mh - 1))) for p in range(4)]


results = []
shapes = [((1000, 1000), np.uint8), ((1000, 1000), np.uint16)] if a.small else [((4000, 6000), np.uint8), ((5792, 8688), np.uint16)]
for (h, w), dt in shapes:
    dt = np.dtype(dt)
    maxv = int(np.iinfo(dt).max)
    black = 4 if dt.itemsize == 1 else 1024
    cfa = demosaic.Cfa(black=black)
    c = cfa.struct(dt)
    code = L.DTYPE_CODE[dt]
    rng = np.random.default_rng(3)
    mosaic = rng.integers(black, maxv // 2, size=(h, w)).astype(dt)
    buf, other = L.DeviceBuffer(mosaic.nbytes), L.DeviceBuffer(mosaic.nbytes)
    buf.upload(mosaic)
    dh, dv = np.arange(w) % 3 - 1, 1 - np.arange(h) % 3
    variants = [("deltas", dng.SiteCorrections(black_h=dh, black_v=dv))]
    for mv, mh in ((13, 17), (257, 257)):
        variants += [(f"gains {mv}x{mh}", dng.SiteCorrections(gains=gain_maps(mv, mh))),
                     (f"both {mv}x{mh}", dng.SiteCorrections(black_h=dh, black_v=dv, gains=gain_maps(mv, mh)))]
    runs = [("copy", lambda: L.check(lib.mi_memcpy_d2d_async(0, None, other.ptr, buf.ptr, mosaic.nbytes)))]
    for name, sc in variants:
        st = sc.prepared((h, w), dt, 0)
        runs.append((name, lambda st=st: L.check(lib.mi_mosaic_site_correct_device(0, None, buf.ptr, h, w, code, C.byref(c), C.byref(st)))))
    for pas in range(2):
        times = {name: measure(fn) for name, fn in runs}
    for name, ms in times.items():
        row = {"shape": [h, w], "dtype": dt.name, "variant": name, "ms": ms, "over_copy": ms / times["copy"],
               "GBps": 2 * mosaic.nbytes / ms / 1e6}
        results.append(row)
        print(f"{h}x{w} {dt.name:6s} {name:16s} {ms:8.4f} ms   x{row['over_copy']:.2f} of the copy   {row['GBps']:7.1f} GB/s", flush=True)
    for _, sc in variants:
        sc.close()
    buf.free()
    other.free()
if a.json:
    with open(a.json, "w") as fh:
        json.dump(results, fh, indent=1)
