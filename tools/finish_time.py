"""Alone on the GPU: the finishing kernels of csrc/kernels_finish.hpp on resident frames of 24 MP uint8 and 50 MP uint16.
mosaic_radial_gain (mi_mosaic_radial_gain_device, in place on the mosaic) beside a device-to-device copy of the mosaic and beside
mosaic_site_correct's deltas-only pass; frame_finish (mi_frame_finish_device, H x W x 3 -> the cropped, oriented frame) beside a
device-to-device copy of the frame, the row orientations (1..4) apart from the transposing ones (5..8).  Every timing sits
beside its copy taken in the same run.

    python tools/finish_time.py [--runs 20] [--small] [--json FILE]

Method, as tools/sitecorr_time.py: hipEvents around 5 back-to-back launches, 3 warm-up launches, the median of `--runs`
windows; the whole list is measured twice and the second pass is reported (the first warms clocks and caches).  The gain
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
PER, WARM = 5, 3        # launches per timed window, warm-up launches


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
    frame_bytes = 3 * mosaic.nbytes
    buf, other = L.DeviceBuffer(mosaic.nbytes), L.DeviceBuffer(mosaic.nbytes)
    src, dst = L.DeviceBuffer(frame_bytes), L.DeviceBuffer(frame_bytes)
    buf.upload(mosaic)
    src.upload(rng.integers(0, maxv, size=(h, w, 3)).astype(dt))
    gain = dng.RadialGain((0.3, 0.1, 0.0, 0.0, 0.0), ((w - 1) / 2.0, (h - 1) / 2.0))
    rg = gain.prepared((h, w), 0)
    deltas = dng.SiteCorrections(black_h=np.arange(w) % 3 - 1, black_v=1 - np.arange(h) % 3)
    st = deltas.prepared((h, w), dt, 0)
    crop = (2, 3, h - 5, w - 7)     # an odd origin: source rows off the 16-byte grid
    runs = [("mosaic copy", mosaic.nbytes, lambda: L.check(lib.mi_memcpy_d2d_async(0, None, other.ptr, buf.ptr, mosaic.nbytes))),
            ("site deltas", mosaic.nbytes, lambda: L.check(lib.mi_mosaic_site_correct_device(0, None, buf.ptr, h, w, code, C.byref(c), C.byref(st)))),
            ("radial gain", mosaic.nbytes, lambda: L.check(lib.mi_mosaic_radial_gain_device(0, None, buf.ptr, h, w, code, C.byref(c), C.byref(rg)))),
            ("frame copy", frame_bytes, lambda: L.check(lib.mi_memcpy_d2d_async(0, None, dst.ptr, src.ptr, frame_bytes)))]
    for o in range(1, 9):
        runs.append((f"finish o{o}", frame_bytes, lambda o=o: L.check(lib.mi_frame_finish_device(0, None, src.ptr, dst.ptr, h, w, code, 0, 0, h, w, o))))
    for o in (1, 2, 6):
        cb = crop[2] * crop[3] * 3 * dt.itemsize
        runs.append((f"finish o{o} crop", cb, lambda o=o: L.check(lib.mi_frame_finish_device(0, None, src.ptr, dst.ptr, h, w, code, *crop, o))))
    for pas in range(2):
        times = {name: measure(fn) for name, _, fn in runs}
    for name, nbytes, _ in runs:
        ms = times[name]
        ref = times["mosaic copy"] if nbytes == mosaic.nbytes else times["frame copy"] * nbytes / frame_bytes
        row = {"shape": [h, w], "dtype": dt.name, "variant": name, "ms": ms, "over_copy": ms / ref, "GBps": 2 * nbytes / ms / 1e6}
        results.append(row)
        print(f"{h}x{w} {dt.name:6s} {name:16s} {ms:8.4f} ms   x{row['over_copy']:.2f} of the copy   {row['GBps']:7.1f} GB/s", flush=True)
    rows = [times[f"finish o{o}"] for o in (1, 2, 3, 4)]
    turns = [times[f"finish o{o}"] for o in (5, 6, 7, 8)]
    print(f"{h}x{w} {dt.name:6s} rows (1..4) median {statistics.median(rows):.4f} ms, transposing (5..8) median {statistics.median(turns):.4f} ms",
          flush=True)
    gain.close()
    deltas.close()
    for b in (buf, other, src, dst):
        b.free()
if a.json:
    with open(a.json, "w") as fh:
        json.dump(results, fh, indent=1)
