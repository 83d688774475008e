#!/usr/bin/env python3
"""Time one brush stroke of 2000 stamps on the device, at radius 25 and at radius 500, on a 24 MP uint8 and a 50 MP uint16 frame.

    python tools/brush_time.py [--reps 5] [--cpu-stamps 12]

Beside each time: a device-to-device copy of as many bytes as the stroke's bounding box holds in one frame (the floor: the
stroke reads two frames' worth of the box and writes one), and the restated stamp loop (tests/brush_restatement.stroke_loop,
what the reference does) on this machine's CPU.  The CPU loop is timed over the stroke's first `--cpu-stamps` stamps and
its per-stamp time scaled to 2000 (the set-up, timed with no stamps, counted once), which the output says.  One JSON line per case.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import brush_restatement as br  # noqa: E402
from shinestacker_amd import _lib, retouch  # noqa: E402

N_STAMPS = 2000


def zigzag(h, w, size, n):
    """n stamp positions along a zigzag over the frame, spaced as the viewer spaces them"""
    pts, y, leg = [(0.05 * w, 0.1 * h)], 0.1 * h, 0
    while True:
        leg += 1
        y = 0.1 * h + (leg * 0.07 * h) % (0.8 * h)
        pts.append((0.95 * w if leg % 2 else 0.05 * w, y))
        stamps = retouch.stamps_along(pts, size)
        if len(stamps) >= n:
            return stamps[:n]


def frame(h, w, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, (h, w, 3), dtype=dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-stamps", type=int, default=12)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    for (h, w), dtype in (((4000, 6000), np.uint8), ((5792, 8688), np.uint16)):
        master, source = frame(h, w, dtype, 1), frame(h, w, dtype, 2)
        m, s, scratch = (_lib.DeviceBuffer(master.nbytes) for _ in range(3))
        s.upload(source)
        for radius in (25, 500):
            size, hardness, opacity, flow = 2 * radius + 1, 50, 100, 30
            stamps = zigzag(h, w, size, N_STAMPS)
            centres = retouch.stamp_centres(stamps)
            box = np.asarray(retouch.stroke_box(centres, radius, h, w), np.int32)
            table = np.ascontiguousarray(retouch.brush_mask(size, hardness, opacity) * flow / 100.0)
            t, c = _lib.DeviceBuffer(table.nbytes), _lib.DeviceBuffer(centres.nbytes)
            t.upload(table)
            c.upload(centres)
            box_bytes = int(box[2] - box[0]) * int(box[3] - box[1]) * 3 * master.dtype.itemsize
            gpu, copy = [], []
            for _ in range(args.reps + 1):
                m.upload(master)
                t0 = time.perf_counter()
                _lib.check(lib.mi_brush_stroke_device(0, None, m.ptr, s.ptr, h, w, _lib.DTYPE_CODE[master.dtype], t.ptr, radius, c.ptr,
                                                      len(centres), box.ctypes.data, opacity / 100.0, None))
                _lib.check(lib.mi_device_synchronize(0))
                gpu.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                _lib.check(lib.mi_memcpy_d2d(0, scratch.ptr, s.ptr, box_bytes))
                _lib.check(lib.mi_device_synchronize(0))
                copy.append(time.perf_counter() - t0)
            k = min(args.cpu_stamps, len(centres))
            first = [tuple(v) for v in centres[:k].tolist()]
            tab, setup = retouch.brush_mask(size, hardness, opacity), None
            for part in ([], first):        # the loop without stamps is its set-up: the copies and the zero mask layer
                t0 = time.perf_counter()
                br.stroke_loop(master, source, tab, part, radius, opacity, flow)
                setup, cpu = (time.perf_counter() - t0, None) if setup is None else (setup, time.perf_counter() - t0)
            cpu = setup + (cpu - setup) * len(centres) / k
            print(json.dumps({"frame": [h, w], "dtype": master.dtype.name, "radius": radius, "stamps": len(centres),
                              "box": box.tolist(), "box_mbytes": round(box_bytes / 1e6, 1),
                              "stroke_ms": round(1e3 * min(gpu[1:]), 3), "stroke_ms_median": round(1e3 * float(np.median(gpu[1:])), 3),
                              "box_copy_ms": round(1e3 * min(copy[1:]), 3),
                              "cpu_stamp_loop_s": round(cpu, 2), "cpu_stamps_timed": k}), flush=True)
            t.free()
            c.free()
        for b in (m, s, scratch):
            b.free()


if __name__ == "__main__":
    main()
