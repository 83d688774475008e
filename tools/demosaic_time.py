"""Alone on the GPU: the demosaic kernel (mi_demosaic_device) on a resident mosaic of 24 MP and of 50 MP uint16, hipEvents over
warm runs, beside a device-to-device copy that moves the same bytes (itemsize read + 3 * itemsize written per pixel =
4 * itemsize: the copy reads and writes half of that each), taken in the same run.  Every line reports the median, the ratio to
that copy and the GB/s of the kernel's bytes.

    python tools/demosaic_time.py [--runs 20] [--uint8] [--small] [--json FILE]
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
from shinestacker_amd import demosaic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--uint8", action="store_true", help="the two shapes at uint8 as well")
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
INNER = 5       # launches per timed window: a single launch of ~0.1 ms would measure the events
results = []


def measure(run):
    for _ in range(3):
        run()
    L.check(lib.mi_device_synchronize(0))
    times = []
    for _ in range(a.runs):
        ck(hip.hipEventRecord(e0, None), "hipEventRecord")
        for _ in range(INNER):
            run()
        ck(hip.hipEventRecord(e1, None), "hipEventRecord")
        ck(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float()
        ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        times.append(ms.value / INNER)
    return statistics.median(times), min(times)


shapes = [("1 MP", 1000, 1000)] if a.small else [("24 MP", 4000, 6000), ("50 MP", 5792, 8640)]
cfa = demosaic.Cfa("RGGB", black=256, gains=[1.9, 1.0, 1.0, 1.5])
for dt in ([np.uint16, np.uint8] if a.uint8 else [np.uint16]):
    dt = np.dtype(dt)
    for name, h, w in shapes:
        px = h * w
        moved = px * 4 * dt.itemsize
        rng = np.random.default_rng(px)
        mosaic = L.DeviceBuffer(px * dt.itemsize)
        mosaic.upload(rng.integers(0, int(np.iinfo(dt).max) + 1, size=(h, w)).astype(dt))
        out = L.DeviceBuffer(px * 3 * dt.itemsize)
        scratch = L.DeviceBuffer(moved)           # source and target of the copy: half of the kernel's bytes each
        half = moved // 2
        copy_ms, _ = measure(lambda: L.check(lib.mi_memcpy_d2d_async(0, None, scratch.ptr, scratch.ptr + half, half)))
        ms, best = measure(lambda: demosaic.debayer_device(mosaic.ptr, out.ptr, h, w, dt, cfa))
        results.append(dict(shape=name, dtype=dt.name, height=h, width=w, median_ms=ms, best_ms=best, copy_ms=copy_ms,
                            ratio_to_copy=ms / copy_ms, bytes=moved, gbps=1e-6 * moved / ms))
        print(f"{name} {dt.name:6s} {w}x{h}: median {ms:7.3f} ms best {best:7.3f} ms over {a.runs} x {INNER} launches | copy of "
              f"{1e-6 * moved:5.0f} MB moved {copy_ms:7.3f} ms | {ms / copy_ms:5.2f} x the copy | {1e-6 * moved / ms:5.0f} GB/s", flush=True)
        for b in (mosaic, out, scratch):
            b.free()
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(results, fh, indent=1)
