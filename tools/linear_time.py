"""Alone on the GPU: linear_develop (mi_linear_develop_device, csrc/kernels_linear.hpp) on a resident LinearRaw frame of 24 MP
uint8 and of 50 MP uint16, three samples per pixel -- plain, with the colour matrix, and with the matrix and the tone table --
beside a device-to-device copy that moves the same bytes (3 * itemsize read + 3 * itemsize written per pixel: the copy reads
and writes half of that each), taken in the same run.  The frame is a smooth scene with 1 % noise, what the uint16 tone
table's gather sees on a photograph; ", random" repeats the tone variant on a uniform random frame, the gather's worst case.
The method is tools/demosaic_time.py's: hipEvents around 5 back-to-back launches, 3 warm-up launches, the median of `--runs`
windows; the whole list is measured twice and the second pass is reported.

    python tools/linear_time.py [--runs 20] [--small] [--json FILE]

Then raw_ljpeg3 (mi_raw_ljpeg3_device, csrc/kernels_ljpeg.hpp) in tiles of 256 x 256 pixels of three components beside raw_ljpeg
on the same plane of samples in tiles of 256 x 768 samples of two components: predictor 1, 12 bits, ljpeg_encode.scene; each
frame is decoded once and compared with the plane before it is timed.
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


camera = [[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [0.05, -0.55, 1.5]]
cases = [("1 MP", 1000, 1000, np.uint8), ("1 MP", 1000, 1000, np.uint16)] if a.small else \
    [("24 MP", 4000, 6000, np.uint8), ("50 MP", 5792, 8640, np.uint16)]
for name, h, w, dt in cases:
    dt = np.dtype(dt)
    mx = int(np.iinfo(dt).max)
    lin = demosaic.Linear(black=1 if dt.itemsize == 1 else 256, gains=[1.9, 1.0, 1.5])
    ls = lin.struct(dt)
    px = h * w
    moved = px * 6 * dt.itemsize
    rng = np.random.default_rng(px)
    smooth = ((0.5 + 0.3 * np.sin(np.arange(w) / 230.0)[None, :] * np.cos(np.arange(h) / 170.0)[:, None]) * mx).astype(np.float32)
    scene = L.DeviceBuffer(px * 3 * dt.itemsize)
    scene.upload(np.clip(smooth[:, :, None] + rng.integers(-mx // 100 - 1, mx // 100 + 2, size=(h, w, 3), dtype=np.int32), 0, mx).astype(dt))
    del smooth
    noise = L.DeviceBuffer(px * 3 * dt.itemsize)
    noise.upload(rng.integers(0, mx + 1, size=(h, w, 3), dtype=np.int32).astype(dt))
    out = L.DeviceBuffer(px * 3 * dt.itemsize)
    scratch = L.DeviceBuffer(moved)           # source and target of the copy: half of the kernel's bytes each
    half = moved // 2
    code = L.DTYPE_CODE[dt]
    devs = {"matrix": demosaic.Develop(matrix=camera), "matrix + tone": demosaic.Develop(matrix=camera, tone="srgb")}
    runs = [("copy", lambda: L.check(lib.mi_memcpy_d2d_async(0, None, scratch.ptr, scratch.ptr + half, half))),
            ("plain", lambda: L.check(lib.mi_linear_develop_device(0, None, scene.ptr, out.ptr, h, w, code, C.byref(ls), None)))]
    for key, dev in devs.items():
        d, _, _ = dev.prepared((h, w), dt)
        runs.append((key, lambda d=d: L.check(lib.mi_linear_develop_device(0, None, scene.ptr, out.ptr, h, w, code, C.byref(ls), C.byref(d)))))
        if key != "matrix":
            runs.append((key + ", random", lambda d=d: L.check(lib.mi_linear_develop_device(0, None, noise.ptr, out.ptr, h, w, code, C.byref(ls),
                                                                                            C.byref(d)))))
    for rep in range(2):
        got = {key: measure(fn) for key, fn in runs}
    copy_ms = got["copy"][0]
    for key, (ms, best) in got.items():
        results.append(dict(shape=name, dtype=dt.name, height=h, width=w, what=key, median_ms=ms, best_ms=best, copy_ms=copy_ms,
                            ratio_to_copy=ms / copy_ms, bytes=moved, gbps=1e-6 * moved / ms))
        print(f"{name} {dt.name:6s} {w}x{h} {key:22s}: median {ms:7.4f} ms best {best:7.4f} ms | {1e-6 * moved / ms:5.0f} GB/s | "
              f"{ms / copy_ms:5.2f} x the copy of {1e-6 * moved:4.0f} MB ({copy_ms:6.4f} ms)", flush=True)
    for d in devs.values():
        d.close()
    for b in (scene, noise, out, scratch):
        b.free()
# ---- raw_ljpeg3 beside raw_ljpeg on the same number of samples: tiles of 256 x 256 pixels (768 samples across) of three
# components against tiles of 256 x 768 samples of two, predictor 1, 12 bits, the same plane of samples (ljpeg_encode.scene)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ljpeg_encode as E  # noqa: E402
from shinestacker_amd import dng  # noqa: E402

HP, WP = (512, 768) if a.small else (2048, 3072)
plane = E.scene(HP, 3 * WP, 12)
out = L.DeviceBuffer(plane.nbytes)
for what, ncomp, spp in (("raw_ljpeg, 2 components", 2, 1), ("raw_ljpeg3, 3 components", 3, 3)):
    span, segs = E.encode_frame(plane, 12, 256, 768, True, ncomp=ncomp)
    lay = dng.RawLayout(12, False, HP, 3 * WP, True, 256, 768, np.zeros(len(segs), np.uint32), compression=7, segments=segs, spp=spp)
    at = (span.nbytes + 255) & ~255
    st_at = at + ((segs.nbytes + 255) & ~255)
    buf = L.DeviceBuffer(st_at + 4 * len(segs))
    buf.upload(span)
    buf.upload(segs, at)
    ms, best = measure(lambda: dng.unpack_device(lay, buf.ptr, span.nbytes, buf.ptr + at, None, out.ptr, dev_status=buf.ptr + st_at))
    assert not buf.download((len(segs),), np.uint32, st_at).any()
    assert np.array_equal(out.download(plane.shape, np.uint16), plane), what + " does not return the samples"
    results.append(dict(what=what, height=HP, width_px=WP, samples=int(plane.size), tiles=len(segs), median_ms=ms, best_ms=best,
                        us_per_sample_of_a_tile=1e3 * ms / (256 * 768), span_over_uint16=span.nbytes / plane.nbytes))
    print(f"{HP} x {WP} px, {plane.size / 1e6:.1f} M samples in {len(segs)} tiles of 256 x 768 samples, {what:26s}: median {ms:8.3f} ms best "
          f"{best:8.3f} ms | {1e3 * ms / (256 * 768):6.3f} us a sample of one tile | span {span.nbytes / plane.nbytes:5.3f} of the uint16 samples",
          flush=True)
    buf.free()
out.free()
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(results, fh, indent=1)
