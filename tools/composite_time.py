"""Alone on the GPU: the depth-selected composite (mi_depth_composite_device) over 32 resident frames of 24 MP uint8 and of
50 MP uint16, both `interp`, on three depth planes, hipEvents over warm runs, each beside a device-to-device copy of as many
bytes as the form's table row says it moves (csrc/kernels_composite.hpp: depth 4, frames 3 s or 6 s, output 3 s per pixel), taken
in the same run.  Every line reports the median, the ratio to that copy and the GB/s of the table-row bytes.

    python tools/composite_time.py [--runs 20] [--frames 32] [--json FILE]

Planes: `smooth` -- the depth map (sigma 2) of a stack of the synthetic generator's frames, which are the frames gathered from;
`constant` -- one fractional index everywhere (every wave takes the fast path); `checker` -- a per-pixel checkerboard between the
first and the last frame (every wave takes the gather path)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shinestacker_amd import _lib as L  # noqa: E402
from shinestacker_amd import depth_render  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--frames", type=int, default=32)
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
N = a.frames
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


shapes = (("1 MP uint8  ", 1000, 1000, np.uint8), ("1 MP uint16 ", 1000, 1000, np.uint16)) if a.small else \
    (("24 MP uint8 ", 4000, 6000, np.uint8), ("50 MP uint16", 5760, 8640, np.uint16))
for name, h, w, dt in shapes:
    dt = np.dtype(dt)
    px = h * w
    fb = px * 3 * dt.itemsize
    frames = L.DeviceBuffer(fb * N)
    out = L.DeviceBuffer(fb)
    depth = L.DeviceBuffer(px * 4)
    scratch = L.DeviceBuffer(2 * (px * 4 + 3 * fb))       # source and target of the copies: the largest table row
    L.synth_frames_device(frames.ptr, dt, h, w, 0, N, N)
    ptrs = [frames.ptr + i * fb for i in range(N)]
    y, x = np.mgrid[0:h, 0:w]
    planes = {"constant": np.full((h, w), np.float32(N // 2 + 0.37), np.float32),
              "checker": np.where((y + x) % 2 == 0, 0.0, float(N - 1)).astype(np.float32)}
    del y, x
    with L.Stack(h, w, in_dtype=dt, out_dtype=dt) as stack:
        stack.push_frames_device(frames.ptr, N, fb)
        stack.sync()
        smooth = stack.depth_map(2.0)
    mixed = float((np.ptp(np.floor(smooth.reshape(-1)[: px // 256 * 256].reshape(-1, 256)), axis=1) > 0).mean())
    print(f"{name} smooth plane: depth map (sigma 2) of the {N} frames, mean {smooth.mean():.2f}; {100 * mixed:.1f} % of the runs of 256 "
          f"pixels hold more than one frame index", flush=True)
    for plane_name, plane in (("smooth", smooth), ("constant", planes["constant"]), ("checker", planes["checker"])):
        depth.upload(plane)
        for interp in ("linear", "nearest"):
            row = px * (4 + (9 if interp == "linear" else 6) * dt.itemsize)        # bytes of the table row
            half = row // 2 // 16 * 16
            copy_ms, _ = measure(lambda: L.check(lib.mi_memcpy_d2d_async(0, None, scratch.ptr, scratch.ptr + scratch.nbytes // 2, half)))
            ms, best = measure(lambda: depth_render.composite_device(ptrs, 0, N, N, depth.ptr, out.ptr, h, w, dt, interp))
            results.append(dict(shape=name.strip(), plane=plane_name, interp=interp, median_ms=ms, best_ms=best, copy_ms=copy_ms,
                                ratio_to_copy=ms / copy_ms, table_row_bytes=row, gbps=1e-6 * row / ms))
            print(f"{name} {plane_name:8s} {interp:7s} median {ms:7.3f} ms best {best:7.3f} ms over {a.runs} x {INNER} launches | copy of "
                  f"{1e-6 * row:6.0f} MB moved {copy_ms:7.3f} ms | {ms / copy_ms:5.2f} x the copy | {1e-6 * row / ms:5.0f} GB/s of the table row",
                  flush=True)
    for b in (frames, out, depth, scratch):
        b.free()
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(results, fh, indent=1)
