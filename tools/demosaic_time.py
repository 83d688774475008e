"""Alone on the GPU: the demosaic kernel (mi_demosaic_device) on a resident mosaic of 24 MP and of 50 MP uint16, hipEvents over
warm runs, beside a device-to-device copy that moves the same bytes (itemsize read + 3 * itemsize written per pixel =
4 * itemsize: the copy reads and writes half of that each), taken in the same run.  Every line reports the median, the ratio to
that copy and the GB/s of the kernel's bytes.

    python tools/demosaic_time.py [--runs 20] [--uint8] [--small] [--json FILE]

`--develop`: raw development instead (24 MP uint8 and 50 MP uint16, resident): the developed kernel with the colour matrix only,
the tone table only and both (mi_develop_device), the defect kernel at 1 000 and at 100 000 sites (mi_mosaic_defects_device,
which repairs the same mosaic in place over and over: the values settle, the work per launch does not change), and, in the same
process on the same frame, the plain demosaic_mhc and a device copy of the same bytes.  The frame is uniform random -- the worst
case for the uint16 tone table's gather -- and the tone variants run once more on a smooth scene with 1 % noise (", scene").  Same method for every line: hipEvents
around 5 back-to-back launches, 3 warm-up launches, the median of `--runs` windows; the whole list is measured twice and the
second pass is reported (the first warms clocks and caches).

`--calibrate`: raw calibration instead (24 MP uint8 and 50 MP uint16, resident), by the same method: the calibration kernel
(mi_mosaic_calibrate_device, in place) with the dark only, the flat only and both, each beside a device-to-device copy that
moves the bytes the variant moves (mosaic read and written, dark read, gains read); and mi_mosaic_master_device over K = 16
frames with reject 0 and reject 7, beside a device copy of the same 16 frames -- a kernel-free read of them, which also writes
them, so twice the master's traffic.
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
ap.add_argument("--develop", action="store_true", help="time raw development: matrix, tone, both, the defect kernel; beside plain and copy")
ap.add_argument("--calibrate", action="store_true", help="time raw calibration: dark, flat, both, the master kernel; beside copies of the same bytes")
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


def develop_section():
    """--develop: every variant on one resident frame per (shape, dtype), two passes, the second reported"""
    camera = [[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [0.05, -0.55, 1.5]]
    cases = [("1 MP", 1000, 1000, np.uint8), ("1 MP", 1000, 1000, np.uint16)] if a.small else \
        [("24 MP", 4000, 6000, np.uint8), ("50 MP", 5792, 8640, np.uint16)]
    for name, h, w, dt in cases:
        dt = np.dtype(dt)
        cfa_d = demosaic.Cfa("RGGB", black=1 if dt.itemsize == 1 else 256, gains=[1.9, 1.0, 1.0, 1.5])
        px = h * w
        moved = px * 4 * dt.itemsize
        rng = np.random.default_rng(px)
        mosaic = L.DeviceBuffer(px * dt.itemsize)
        mosaic.upload(rng.integers(0, int(np.iinfo(dt).max) + 1, size=(h, w)).astype(dt))
        # ... and a smooth scene with 1 % noise: neighbouring pixels index neighbouring tone entries, which is what the uint16
        # table's gather sees on a photograph (the uniform random mosaic is its worst case: 64 cache lines per wave and load)
        mx = int(np.iinfo(dt).max)
        scene = L.DeviceBuffer(px * dt.itemsize)
        smooth = (0.5 + 0.3 * np.sin(np.arange(w) / 230.0)[None, :] * np.cos(np.arange(h) / 170.0)[:, None]) * mx
        scene.upload(np.clip(smooth + rng.integers(-mx // 100 - 1, mx // 100 + 2, size=(h, w)), 0, mx).astype(dt))
        del smooth
        out = L.DeviceBuffer(px * 3 * dt.itemsize)
        scratch = L.DeviceBuffer(moved)
        half = moved // 2
        code = L.DTYPE_CODE[dt]

        def sites(n):
            return np.stack(np.divmod(np.unique(rng.integers(0, px, size=n)), w), axis=1)   # (a handful fewer where draws repeat)

        devs = {"matrix": demosaic.Develop(matrix=camera), "tone": demosaic.Develop(tone="srgb"),
                "matrix + tone": demosaic.Develop(matrix=camera, tone="srgb"),
                "defects 1 000": demosaic.Develop(defects=sites(1000)), "defects 100 000": demosaic.Develop(defects=sites(100000))}
        runs = [("copy", lambda: L.check(lib.mi_memcpy_d2d_async(0, None, scratch.ptr, scratch.ptr + half, half))),
                ("plain", lambda: demosaic.debayer_device(mosaic.ptr, out.ptr, h, w, dt, cfa_d))]
        for key in ("matrix", "tone", "matrix + tone"):
            d, _, _ = devs[key].prepared((h, w), dt)
            c = cfa_d.struct(dt)
            runs.append((key, lambda d=d, c=c: L.check(lib.mi_develop_device(0, None, mosaic.ptr, out.ptr, h, w, code, C.byref(c), C.byref(d)))))
            if key != "matrix":
                runs.append((key + ", scene", lambda d=d, c=c: L.check(lib.mi_develop_device(0, None, scene.ptr, out.ptr, h, w, code, C.byref(c), C.byref(d)))))
        for key in ("defects 1 000", "defects 100 000"):
            _, ptr, n = devs[key].prepared((h, w), dt)
            runs.append((key, lambda ptr=ptr, n=n: L.check(lib.mi_mosaic_defects_device(0, None, mosaic.ptr, h, w, code, ptr, n))))
        for rep in range(2):
            got = {key: measure(fn) for key, fn in runs}
        copy_ms, plain_ms = got["copy"][0], got["plain"][0]
        for key, (ms, best) in got.items():
            results.append(dict(shape=name, dtype=dt.name, height=h, width=w, what=key, median_ms=ms, best_ms=best, copy_ms=copy_ms,
                                ratio_to_copy=ms / copy_ms, ratio_to_plain=ms / plain_ms))
            print(f"{name} {dt.name:6s} {w}x{h} {key:20s}: median {ms:7.4f} ms best {best:7.4f} ms | {ms / plain_ms:5.2f} x plain | "
                  f"{ms / copy_ms:5.2f} x the copy of {1e-6 * moved:4.0f} MB ({copy_ms:6.4f} ms)", flush=True)
        for d in devs.values():
            d.close()
        for b in (mosaic, scene, out, scratch):
            b.free()


def calibrate_section():
    """--calibrate: every variant on one resident frame per (shape, dtype), two passes, the second reported"""
    K = 16
    cases = [("1 MP", 1000, 1000, np.uint8), ("1 MP", 1000, 1000, np.uint16)] if a.small else \
        [("24 MP", 4000, 6000, np.uint8), ("50 MP", 5792, 8640, np.uint16)]
    for name, h, w, dt in cases:
        dt = np.dtype(dt)
        mx = int(np.iinfo(dt).max)
        cfa_c = demosaic.Cfa("RGGB", black=1 if dt.itemsize == 1 else 256)
        c = cfa_c.struct(dt)
        px, code = h * w, L.DTYPE_CODE[dt]
        rng = np.random.default_rng(px)
        frames = L.DeviceBuffer(K * px * dt.itemsize)          # the mosaic under calibration is frame 0
        first = rng.integers(0, mx + 1, size=(h, w)).astype(dt)
        for k in range(K):
            frames.upload(np.roll(first, 977 * k, axis=1), k * px * dt.itemsize)
        del first
        dark, gain = L.DeviceBuffer(px * dt.itemsize), L.DeviceBuffer(px * 2)
        dark.upload(rng.integers(0, mx // 8, size=(h, w)).astype(dt))
        gain.upload(rng.integers(12000, 45000, size=(h, w)).astype(np.uint16))
        master = L.DeviceBuffer(px * dt.itemsize)
        scratch = L.DeviceBuffer(K * px * dt.itemsize)
        moved = {"dark": 3 * px * dt.itemsize, "flat": 2 * px * dt.itemsize + 2 * px, "dark + flat": 3 * px * dt.itemsize + 2 * px,
                 "master": (K + 1) * px * dt.itemsize}
        flags = {"dark": L.MI_CALIB_DARK, "flat": L.MI_CALIB_FLAT, "dark + flat": L.MI_CALIB_DARK | L.MI_CALIB_FLAT}
        runs = []
        for key, fl in flags.items():
            cal = L.CalibStruct(fl, dark.ptr, gain.ptr)
            half = moved[key] // 2
            runs.append(("copy for " + key, lambda half=half: L.check(lib.mi_memcpy_d2d_async(0, None, scratch.ptr, scratch.ptr + half, half))))
            runs.append((key, lambda cal=cal: L.check(lib.mi_mosaic_calibrate_device(0, None, frames.ptr, h, w, code, C.byref(c), C.byref(cal)))))
        runs.append(("copy of the 16 frames", lambda: L.check(lib.mi_memcpy_d2d_async(0, None, scratch.ptr, frames.ptr, K * px * dt.itemsize))))
        for reject in (0, 7):
            runs.append((f"master K=16 reject {reject}",
                         lambda reject=reject: L.check(lib.mi_mosaic_master_device(0, None, frames.ptr, K, h, w, code, reject, master.ptr))))
        for rep in range(2):
            got = {key: measure(fn) for key, fn in runs}
        for key, (ms, best) in got.items():
            if key.startswith("copy"):
                continue
            ref = "copy of the 16 frames" if key.startswith("master") else "copy for " + key
            nbytes = moved["master"] if key.startswith("master") else moved[key]
            copy_ms = got[ref][0]
            results.append(dict(shape=name, dtype=dt.name, height=h, width=w, what=key, median_ms=ms, best_ms=best, copy_ms=copy_ms,
                                ratio_to_copy=ms / copy_ms, bytes=nbytes, gbps=1e-6 * nbytes / ms))
            print(f"{name} {dt.name:6s} {w}x{h} {key:22s}: median {ms:7.4f} ms best {best:7.4f} ms | {1e-6 * nbytes:5.0f} MB at "
                  f"{1e-6 * nbytes / ms:5.0f} GB/s | {ms / copy_ms:5.2f} x its copy ({ref}: {copy_ms:6.4f} ms)", flush=True)
        for b in (frames, dark, gain, master, scratch):
            b.free()


if a.develop:
    develop_section()
if a.calibrate:
    calibrate_section()
for dt in ([] if a.develop or a.calibrate else [np.uint16, np.uint8] if a.uint8 else [np.uint16]):
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
