"""Alone on the GPU: one stereo view (mi_stereo_view_device) and one anaglyph pair (two views + the channel merge) on a 24 MP
uint8 and a 50 MP uint16 frame, hipEvents over warm runs, each against a device-to-device copy of the same frame taken in the
same run.  A view moves 10 B/px (uint8) / 16 B/px (uint16) -- depth 4, image in and out 3 samples each -- against the copy's
6 / 12; every line reports the ratio to the copy and the GB/s of the bytes the form moves.

    python tools/stereo_time.py [--runs 20] [--shift 24]

Frame: the synthetic stack generator's; depth: frame-number bands with a smooth ramp across and hash noise, so that there are
occlusions and holes in every segment (8 frames)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shinestacker_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--shift", type=float, default=24.0)
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
N = 8

for name, h, w, dt in (("24 MP uint8 ", 4000, 6000, np.uint8), ("50 MP uint16", 5760, 8640, np.uint16)):
    dt = np.dtype(dt)
    fb = h * w * 3 * dt.itemsize
    img, left, right, out = (L.DeviceBuffer(fb) for _ in range(4))
    depth = L.DeviceBuffer(h * w * 4)
    L.synth_frames_device(img.ptr, dt, h, w, 0, 1, N)
    y, x = np.mgrid[0:h, 0:w].astype(np.uint32)
    v = (x * np.uint32(0x9E3779B1) ^ y * np.uint32(0x85EBCA77)) >> np.uint32(20)
    z = ((y // 250 + x // 330) % N).astype(np.float32) + (x.astype(np.float32) / w - 0.5) + (v % 64).astype(np.float32) / 128
    depth.upload(np.clip(z, 0, N - 1).astype(np.float32))
    del y, x, v, z
    code = L.DTYPE_CODE[dt]
    copy_ms = None

    def measure(what, nbytes, run):
        global copy_ms
        for _ in range(3):
            run()
        L.check(lib.mi_device_synchronize(0))
        times = []
        for _ in range(a.runs):
            ck(hip.hipEventRecord(e0, None), "hipEventRecord")
            run()
            ck(hip.hipEventRecord(e1, None), "hipEventRecord")
            ck(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float()
            ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            times.append(ms.value)
        mean = sum(times) / len(times)
        if copy_ms is None:
            copy_ms = mean
        print(f"{name} {what:44s} mean {mean:7.3f} ms best {min(times):7.3f} ms over {a.runs} runs | {mean / copy_ms:5.2f} x the copy | "
              f"{1e-6 * nbytes / mean:5.0f} GB/s of the bytes it moves", flush=True)

    def view(dst, shift):
        L.check(lib.mi_stereo_view_device(0, None, img.ptr, depth.ptr, dst, h, w, code, N, shift, 0.5, 0))

    def pair():
        view(left.ptr, a.shift / 2)
        view(right.ptr, -a.shift / 2)
        L.check(lib.mi_stereo_compose_device(0, None, left.ptr, right.ptr, out.ptr, h, w, code, 2))

    px = h * w
    measure("device-to-device copy of the frame", 2.0 * fb, lambda: L.check(lib.mi_memcpy_d2d_async(0, None, out.ptr, img.ptr, fb)))
    measure(f"view, shift {a.shift:g}", px * 4.0 + 2.0 * fb, lambda: view(out.ptr, a.shift))
    measure("view, shift 64", px * 4.0 + 2.0 * fb, lambda: view(out.ptr, 64.0))
    measure(f"anaglyph pair, separation {a.shift:g}", 2 * (px * 4.0 + 2.0 * fb) + 3.0 * fb, pair)
    for b in (img, left, right, out, depth):
        b.free()
