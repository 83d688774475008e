"""Alone on the GPU: the device JPEG decoder (jpeg.decode_device) at 24 MP and 50 MP, 4:4:4 and 4:2:0, quality 95, one
restart interval per MCU row -- frames this tool writes itself, through Pillow, from a seeded scene (a smooth field with
texture and noise; random samples do not compress and would misstate sizes and times).  Warm, in one run:

    entropy            jpeg_entropy alone (mi_jpeg_coefficients_device)
    decode             entropy + inverse DCT + upsampling and colour (mi_jpeg_decode_device); render = decode - entropy
    upload span        the scan's bytes out of pinned memory
    upload BGR         the decoded frame's bytes out of pinned memory: what the host path sends instead
    read_img           the same file through imageio.read_img on one host core (median of 3)
    symbols            DC + non-zero AC + end-of-block symbols of the longest interval, counted from the coefficients, and the
                       entropy time over that count: the serial walk's time per symbol

and, with --stack N, PyramidStack.focus_stack over N copies of the 24 MP 4:4:4 file with jpeg=None and jpeg="device" at
decode_threads=8.  Every frame is decoded once and compared with read_img before it is timed.  Each kernel figure is the
median over `--rounds` rounds of `--reps` back-to-back calls that end in a device synchronise.  --profile: a few decodes of
each frame and nothing else, for a run under `rocprofv3 --kernel-trace --stats`.

--split: the split decoder (csrc/kernels_jpeg_split.hpp) instead.  The same pictures written WITHOUT restart markers, as Pillow
writes them by default, through mi_jpeg_split_coefficients_device / mi_jpeg_split_decode_device at 8, 32 and 128 bytes a
subsequence; the rounds across workgroups each needs, found on the device (the smallest max_rounds of 1, 2, 4, ... after which
no status word says UNSYNCED; 0 where the first launch already has none with one round); the files WITH one interval per MCU
row through split="always", beside jpeg_entropy on the same file (the yardstick) and read_img on one host core; and, with
--stack N, focus_stack over N files without restart markers with jpeg="device", jpeg_split=True against jpeg=None.  With
--profile: three decodes of each plain file at the default options, for the kernel times per pass.
   python tools/jpeg_time.py [--reps 3] [--rounds 5] [--small] [--stack 32] [--profile] [--json] [--split]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shinestacker_amd import _lib as L, jpeg  # noqa: E402
from shinestacker_amd.imageio import read_img  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--small", action="store_true", help="6 MP only: a quick look")
ap.add_argument("--stack", type=int, default=0, help="also time focus_stack over this many copies of the 24 MP 4:4:4 file")
ap.add_argument("--profile", action="store_true")
ap.add_argument("--json", action="store_true")
ap.add_argument("--split", action="store_true", help="time the split decoder on files without restart markers")
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


def pinned(arr):
    p = L.host_alloc(arr.shape, arr.dtype)
    p[...] = arr
    return p


def scene(h, w, seed=0):
    """RGB uint8: smooth gradients, a fine texture and noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([120 + 80 * np.sin(x / 301) * np.cos(y / 173), 110 + 70 * np.cos(x / 97 + y / 211), 90 + 60 * np.sin(y / 59)], -1)
    base += 25 * np.sin(x / 3.1 + y / 4.3)[..., None]
    base += rng.normal(0, 4, (h, w, 3)).astype(np.float32)
    return np.clip(base, 0, 255).astype(np.uint8)


def write(path, rgb, subsampling, rows=True):
    from PIL import Image
    Image.fromarray(rgb).save(path, "JPEG", quality=95, subsampling=subsampling, **({"restart_marker_rows": 1} if rows else {}))


class _Quiet:
    id, name = 0, "quiet"

    def sub_message_r(self, *x, **k):
        pass

    def callback(self, *x, **k):
        return None


def split_times(tmp):
    for H, W in (((2000, 3000),) if a.small else ((4000, 6000), (5792, 8688))):
        rgb = scene(H, W)
        for sub, mode in ((0, "4:4:4"), (2, "4:2:0")):
            plain, rows = os.path.join(tmp, f"p_{H}_{sub}.jpg"), os.path.join(tmp, f"r_{H}_{sub}.jpg")
            write(plain, rgb, sub, rows=False)
            write(rows, rgb, sub)
            host = read_img(plain)
            assert np.array_equal(host, read_img(rows))
            out = L.DeviceBuffer(H * W * 3)
            slot = jpeg.Slot(0)
            res = {}
            try:
                def check(frame):
                    jpeg.decode_device(frame, out.ptr, slot)
                    lib.mi_device_synchronize(0)
                    st = jpeg.settle(frame, out.ptr, slot)
                    assert not st.any(), st
                    assert np.array_equal(out.download((H, W, 3), np.uint8), host), "the device frame differs from read_img's"

                def calls(frame):
                    d, o = L.C.byref(frame.desc), L.C.byref(jpeg._split_opt(frame))
                    args = (0, None, slot.buf.ptr, slot.span_bytes, slot.buf.ptr + slot.off_at, d)
                    if not frame.split:
                        return (lambda: L.check(lib.mi_jpeg_coefficients_device(*args, slot.scratch.ptr, slot.buf.ptr + slot.status_at)),
                                lambda: L.check(lib.mi_jpeg_decode_device(*args, slot.scratch.ptr, slot.scratch.nbytes, out.ptr,
                                                                          slot.buf.ptr + slot.status_at)))
                    return (lambda: L.check(lib.mi_jpeg_split_coefficients_device(*args, o, slot.scratch.ptr, slot.scratch.nbytes, slot.scratch.ptr,
                                                                                  slot.buf.ptr + slot.status_at)),
                            lambda: L.check(lib.mi_jpeg_split_decode_device(*args, o, slot.scratch.ptr, slot.scratch.nbytes, out.ptr,
                                                                            slot.buf.ptr + slot.status_at)))
                frame = jpeg.read(plain, split="needed")
                if a.profile:
                    check(frame)
                    for _ in range(3):
                        calls(frame)[1]()
                    lib.mi_device_synchronize(0)
                    continue
                needed = {}
                for sb in (8, 32, 128):
                    r = 1
                    while True:
                        frame.split_options = (sb, r)
                        jpeg.decode_device(frame, out.ptr, slot)
                        lib.mi_device_synchronize(0)
                        if not (slot.status() & L.JPEG_UNSYNCED).any():
                            break
                        r *= 2
                    needed[sb] = r
                    frame.split_options = (sb, r)
                    check(frame)
                    entropy, decode = calls(frame)
                    res[f"split entropy, {sb} B, {r} rounds"] = median_us(entropy)
                    res[f"split decode,  {sb} B, {r} rounds"] = median_us(decode)
                frame.split_options = (0, 0)
                check(frame)
                res["split decode, defaults"] = median_us(calls(frame)[1])
                always, serial = jpeg.read(rows, split="always"), jpeg.read(rows)
                for name, f in (("rows, split entropy", always), ("rows, jpeg_entropy", serial)):
                    check(f)
                    entropy, decode = calls(f)
                    res[name] = median_us(entropy)
                    res[name.replace("entropy", "decode")] = median_us(decode)
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    read_img(plain)
                    t.append((time.perf_counter() - t0) * 1e6)
                res["read_img, one core"] = (float(np.median(t)), min(t), max(t))
                print(f"{H} x {W} ({H * W / 1e6:.1f} MP) {mode}: file {os.path.getsize(plain) / 1e6:.1f} MB without restart markers, "
                      f"rounds needed {needed}; {a.rounds} rounds of {a.reps}: median (min .. max) us", flush=True)
                for name, r in res.items():
                    print(f"  {name:34s} {r[0]:12.1f} ({r[1]:12.1f} .. {r[2]:12.1f})", flush=True)
                if a.json:
                    print(json.dumps({"height": H, "width": W, "mode": mode, "file_bytes": os.path.getsize(plain), "rounds_needed": needed,
                                      "median_us": {k: round(v[0], 1) for k, v in res.items()}}), flush=True)
            finally:
                lib.mi_device_synchronize(0)
                out.free()
                slot.free()
            if a.stack and (H, W, sub) == ((2000, 3000, 0) if a.small else (4000, 6000, 0)) and not a.profile:
                from shinestacker_amd import PyramidStack
                paths = []
                for i in range(a.stack):
                    paths.append(os.path.join(tmp, f"s{i:03d}.jpg"))
                    shutil.copyfile(plain, paths[-1])
                for kw in ({}, {"jpeg": "device", "jpeg_split": True}, {}, {"jpeg": "device", "jpeg_split": True}):
                    algo = PyramidStack(decode_threads=8, **kw)
                    algo.process = _Quiet()
                    try:
                        t0 = time.perf_counter()
                        algo.focus_stack(paths)
                        dt = time.perf_counter() - t0
                        assert algo.skipped == []
                    finally:
                        algo.close()
                    print(f"  focus_stack over {a.stack} files without restart markers, decode_threads=8, {kw or 'jpeg=None'}: {dt:.2f} s", flush=True)
                for p in paths:
                    os.remove(p)


tmp = tempfile.mkdtemp(prefix="jpeg_time_")
try:
    if a.split:
        split_times(tmp)
        raise SystemExit(0)
    for H, W in (((2000, 3000),) if a.small else ((4000, 6000), (5792, 8688))):
        rgb = scene(H, W)
        for sub, mode in ((0, "4:4:4"), (2, "4:2:0")):
            path = os.path.join(tmp, f"f_{H}_{sub}.jpg")
            write(path, rgb, sub)
            frame = jpeg.read(path)
            host = read_img(path)
            out = L.DeviceBuffer(H * W * 3)
            slot = jpeg.Slot(0)
            res = {}
            try:
                jpeg.decode_device(frame, out.ptr, slot)
                lib.mi_device_synchronize(0)
                assert not slot.status().any()
                assert np.array_equal(out.download((H, W, 3), np.uint8), host), "the device frame differs from read_img's"
                d = L.C.byref(frame.desc)
                args = (0, None, slot.buf.ptr, slot.span_bytes, slot.buf.ptr + slot.off_at, d)

                def entropy():
                    L.check(lib.mi_jpeg_coefficients_device(*args, slot.scratch.ptr, slot.buf.ptr + slot.status_at))

                def decode():
                    L.check(lib.mi_jpeg_decode_device(*args, slot.scratch.ptr, slot.scratch.nbytes, out.ptr, slot.buf.ptr + slot.status_at))
                if a.profile:
                    for _ in range(3):
                        decode()
                    lib.mi_device_synchronize(0)
                    continue
                res["entropy"] = median_us(entropy)
                res["decode"] = median_us(decode)
                hs, hb = pinned(np.ascontiguousarray(frame.span)), pinned(host)
                res["upload span"] = median_us(lambda: L.check(lib.mi_memcpy_h2d(0, slot.buf.ptr, hs.ctypes.data, hs.nbytes)))
                res["upload BGR"] = median_us(lambda: L.check(lib.mi_memcpy_h2d(0, out.ptr, hb.ctypes.data, hb.nbytes)))
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    read_img(path)
                    t.append((time.perf_counter() - t0) * 1e6)
                res["read_img, one core"] = (float(np.median(t)), min(t), max(t))
                # the symbols of the longest interval (one MCU row)
                planes, _ = jpeg.coefficients(frame)
                per = np.zeros(frame.n_intervals, np.int64)
                for c, p in enumerate(planes):
                    v = frame.sampling[1] if c == 0 else 1
                    cnt = np.count_nonzero(p[:, :, 1:], axis=(1, 2)) + 2 * p.shape[1]      # non-zero AC, + DC and EOB per block
                    per += cnt.reshape(frame.n_intervals, v).sum(axis=1)
                longest = int(per.max())
                del planes
                print(f"{H} x {W} ({H * W / 1e6:.1f} MP) {mode}: file {os.path.getsize(path) / 1e6:.1f} MB, {frame.n_intervals} intervals, "
                      f"{a.rounds} rounds of {a.reps}: median (min .. max) us", flush=True)
                for name, r in res.items():
                    print(f"  {name:22s} {r[0]:12.1f} ({r[1]:12.1f} .. {r[2]:12.1f})", flush=True)
                print(f"  render = decode - entropy {res['decode'][0] - res['entropy'][0]:10.1f}", flush=True)
                print(f"  symbols: {int(per.sum())} in all, {longest} in the longest interval: {res['entropy'][0] / longest * 1e3:.1f} ns a symbol there",
                      flush=True)
                if a.json:
                    print(json.dumps({"height": H, "width": W, "mode": mode, "file_bytes": os.path.getsize(path), "intervals": frame.n_intervals,
                                      "median_us": {k: round(v[0], 1) for k, v in res.items()}, "symbols": int(per.sum()),
                                      "longest_interval_symbols": longest}), flush=True)
            finally:
                lib.mi_device_synchronize(0)
                out.free()
                slot.free()
            if a.stack and (H, W, sub) == (4000, 6000, 0) and not a.profile:
                from shinestacker_amd import PyramidStack
                paths = []
                for i in range(a.stack):
                    paths.append(os.path.join(tmp, f"s{i:03d}.jpg"))
                    shutil.copyfile(path, paths[-1])
                for mode_ in (None, "device", None, "device"):
                    algo = PyramidStack(jpeg=mode_, decode_threads=8)
                    algo.process = _Quiet()
                    try:
                        t0 = time.perf_counter()
                        algo.focus_stack(paths)
                        dt = time.perf_counter() - t0
                    finally:
                        algo.close()
                    print(f"  focus_stack over {a.stack} files, decode_threads=8, jpeg={mode_!r}: {dt:.2f} s", flush=True)
                for p in paths:
                    os.remove(p)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
