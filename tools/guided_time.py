"""Alone on the GPU: the depth refinement (mi_depth_guided_device, csrc/kernels_guided.hpp) on a 24 MP uint8 and a 50 MP uint16
guide, radius 6 and 32, float32 weights, hipEvents over warm runs, each beside a device-to-device copy of the same p, w and
guide bytes taken in the same run.  Every line reports the median, the ratio to that copy, and the GB/s of the bytes the
kernels' header counts per pixel (4 launches: p 4 + w 4 + guide 3 s read and 40 written; 40 + 4 read, 16 written; 16 read,
16 written; 16 + 3 s read, 4 written: 160 + 6 s bytes, s the guide's sample size).

    python tools/guided_time.py [--runs 20] [--json FILE] [--small]

The planes: p a step of frame numbers across the middle column with seeded noise, w seeded energies with a zero-weight
quarter, the guide one of the synthetic generator's frames.  The scratch planes are allocated once, outside the timed window."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shinestacker_amd import _lib as L  # noqa: E402
from shinestacker_amd import depth_out  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--json", default=None)
ap.add_argument("--small", action="store_true", help="a 1 MP rehearsal of the whole script")
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
INNER = 5       # calls per timed window
N_FRAMES = 16
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


shapes = (("1 MP uint8  ", 1000, 1000, np.uint8), ("1 MP uint16 ", 1000, 1000, np.uint16)) if a.small else \
    (("24 MP uint8 ", 4000, 6000, np.uint8), ("50 MP uint16", 5760, 8640, np.uint16))
for name, h, w, dt in shapes:
    dt = np.dtype(dt)
    px = h * w
    gb = px * 3 * dt.itemsize
    inputs = px * 8 + gb                                    # p, w and the guide
    rng = np.random.default_rng(h)
    p = (np.where(np.arange(w)[None, :] < w // 2, 3.0, 12.0) + rng.integers(-2, 3, (h, w))).astype(np.float32)
    wt = (rng.random((h, w), np.float32) * 50.0).astype(np.float32)
    wt[: h // 2, : w // 2] = 0
    bufs = [L.DeviceBuffer(n) for n in (px * 4, px * 4, gb, px * 4, depth_out.SCRATCH_PLANES * px * 8, inputs)]
    dp, dw, dg, dout, scratch, mirror = bufs
    dp.upload(p)
    dw.upload(wt)
    L.synth_frames_device(dg.ptr, dt, h, w, N_FRAMES // 2, 1, N_FRAMES)
    del p, wt

    def copy_inputs():
        at = 0
        for b in (dp, dw, dg):
            L.check(lib.mi_memcpy_d2d_async(0, None, mirror.ptr + at, b.ptr, b.nbytes))
            at += b.nbytes
    copy_ms, _ = measure(copy_inputs)
    for radius in (6, 32):
        moved = px * (160 + 6 * dt.itemsize)
        ms, best = measure(lambda: depth_out.guided_refine_device(dp.ptr, dw.ptr, np.float32, dg.ptr, dt, h, w, dout.ptr, 0.0,
                                                                  float(N_FRAMES - 1), radius, 1e-4, scratch_ptr=scratch.ptr))
        results.append(dict(shape=name.strip(), radius=radius, median_ms=ms, best_ms=best, copy_ms=copy_ms, ratio_to_copy=ms / copy_ms,
                            counted_bytes=moved, gbps=1e-6 * moved / ms))
        print(f"{name} radius {radius:2d} median {ms:7.3f} ms best {best:7.3f} ms over {a.runs} x {INNER} calls | copy of the "
              f"{1e-6 * inputs:5.0f} MB of p, w and guide {copy_ms:6.3f} ms | {ms / copy_ms:6.2f} x the copy | {1e-6 * moved / ms:5.0f} GB/s "
              f"of the {moved // px} counted bytes per pixel", flush=True)
    for b in bufs:
        b.free()
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(results, fh, indent=1)
