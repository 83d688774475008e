"""Alone on the GPU: raw_ljpeg (mi_raw_ljpeg_device) at 24 MP and 50 MP for 12 and 14-bit samples, stored as 256 x 256 tiles in
two components with predictor 1 (the form a converter writes) and as strips of 64 rows, warm, beside raw_unpack of the same
samples uncompressed, a device copy of the OUTPUT's bytes, and the upload of each form's bytes out of pinned memory, all timed
in the same run.  Also: the compressed size as a fraction of the uint16 mosaic.

The content is ljpeg_encode.scene: a smooth field with sensor-like shot and read noise on a 2 x 2 colour cell (see there);
random samples do not compress and would misstate both sizes and times.  Every compressed frame is decoded once and compared
with the mosaic it was made from before it is timed.  Each figure is the median over `--rounds` rounds of `--reps`
back-to-back launches that end in a device synchronise.
`--split`: the split path (mi_raw_ljpeg_split_device: decode inside a segment, csrc/kernels_ljpeg_split.hpp) beside the serial
kernel on the same files in the same run, 12-bit samples, and a third segmentation, the whole frame as ONE strip (the serial
kernel is then timed once: one walk of the whole frame).  Per file also: the split path up to the difference plane alone
(mi_ljpeg_split_differences_device: tables, rounds, counts and the write pass -- the rest of the full time is the predict
kernels), the rounds enqueued (the exact bound) and the smallest max_rounds that leaves no segment unsynced.
   python tools/ljpeg_time.py [--reps 5] [--rounds 5] [--small] [--json] [--split]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ljpeg_encode as E  # noqa: E402
from shinestacker_amd import _lib as L, dng  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--small", action="store_true", help="6 MP only: a quick look")
ap.add_argument("--json", action="store_true", help="print one JSON line per frame size as well")
ap.add_argument("--split", action="store_true", help="the split path beside the serial kernel; 12-bit samples, one strip as well")
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


for H, W in (((2000, 3000),) if a.small else ((4000, 6000), (5792, 8688))):
    ob = H * W * 2
    out, src = L.DeviceBuffer(ob), L.DeviceBuffer(ob)
    res, sizes, rounds_info = {}, {}, {}
    try:
        res["copy of the output"] = median_us(lambda: L.check(lib.mi_memcpy_d2d_async(0, None, out.ptr, src.ptr, ob)))
        for bits in ((12,) if a.split else (12, 14)):
            mosaic = E.scene(H, W, bits)
            host = pinned(mosaic)
            res[f"{bits}-bit upload of the uint16 mosaic"] = median_us(lambda: L.check(lib.mi_memcpy_h2d(0, src.ptr, host.ctypes.data, ob)))
            # the same samples packed: strips of 64 rows
            rowb = (W * bits + 7) // 8
            offsets = (np.arange(-(-H // 64), dtype=np.uint64) * (64 * rowb)).astype(np.uint32)
            bit = np.unpackbits(mosaic.byteswap().view(np.uint8).reshape(H, W, 2), axis=2)[:, :, 16 - bits:].reshape(H, W * bits)
            packed = np.packbits(np.concatenate([bit, np.zeros((H, rowb * 8 - W * bits), np.uint8)], axis=1), axis=1).reshape(-1)
            del bit
            lay = dng.RawLayout(bits, False, H, W, False, 64, W, offsets)
            at = (packed.nbytes + 255) & ~255
            buf = L.DeviceBuffer(at + offsets.nbytes)
            try:
                hp = pinned(packed)
                res[f"{bits}-bit upload of the packed span"] = median_us(lambda: L.check(lib.mi_memcpy_h2d(0, buf.ptr, hp.ctypes.data, hp.nbytes)))
                buf.upload(offsets, at)
                res[f"{bits}-bit raw_unpack strips"] = median_us(lambda: dng.unpack_device(lay, buf.ptr, packed.nbytes, buf.ptr + at, None, out.ptr))
                assert np.array_equal(out.download((H, W), np.uint16), mosaic)
            finally:
                buf.free()
            sizes[f"{bits}-bit packed"] = packed.nbytes / ob
            del packed, hp
            kinds = (("tiles 256 x 256", (256, 256, True)), ("strips of 64", (64, W, False)))
            for kind, (sh, sw, tiled) in kinds + ((("one strip", (H, W, False)),) if a.split else ()):
                span, segs = E.encode_frame(mosaic, bits, sh, sw, tiled)
                clay = dng.RawLayout(bits, False, H, W, tiled, sh, sw, np.zeros(len(segs), np.uint32), compression=7, segments=segs)
                at = (span.nbytes + 255) & ~255
                st_at = at + ((segs.nbytes + 255) & ~255)
                buf = L.DeviceBuffer(st_at + 4 * len(segs))
                try:
                    hs = pinned(span)
                    res[f"{bits}-bit upload of the ljpeg span, {kind}"] = median_us(
                        lambda: L.check(lib.mi_memcpy_h2d(0, buf.ptr, hs.ctypes.data, hs.nbytes)))
                    buf.upload(segs, at)

                    def run():
                        dng.unpack_device(clay, buf.ptr, span.nbytes, buf.ptr + at, None, out.ptr, dev_status=buf.ptr + st_at)
                    if kind == "one strip":     # (seconds a launch: timed once)
                        lib.mi_device_synchronize(0)
                        t0 = time.perf_counter()
                        run()
                        lib.mi_device_synchronize(0)
                        res[f"{bits}-bit raw_ljpeg {kind}"] = (float((time.perf_counter() - t0) * 1e6),) * 3
                    else:
                        res[f"{bits}-bit raw_ljpeg {kind}"] = median_us(run)
                    assert not buf.download((len(segs),), np.uint32, st_at).any()
                    assert np.array_equal(out.download((H, W), np.uint16), mosaic), "raw_ljpeg does not return the mosaic"
                    if a.split:
                        Ls = clay.struct()
                        opt, _ = dng.split_options(clay, span.nbytes, True)     # (max_rounds: the exact bound)
                        _, need = dng.split_options(clay, span.nbytes, {"max_rounds": 0xFFFFFFFF})
                        scratch, plane = L.DeviceBuffer(need), L.DeviceBuffer(len(segs) * sh * sw * 2)
                        try:
                            out.upload(np.zeros(ob, np.uint8))        # (the serial kernel's result is not what is compared)

                            def run_split(o=opt):
                                L.check(lib.mi_raw_ljpeg_split_device(0, None, buf.ptr, span.nbytes, buf.ptr + at, L.C.byref(Ls), None, L.C.byref(o),
                                                                      scratch.ptr, scratch.nbytes, out.ptr, buf.ptr + st_at))

                            def run_walk():
                                L.check(lib.mi_ljpeg_split_differences_device(0, None, buf.ptr, span.nbytes, buf.ptr + at, L.C.byref(Ls), L.C.byref(opt),
                                                                              scratch.ptr, scratch.nbytes, plane.ptr, buf.ptr + st_at))
                            res[f"{bits}-bit split {kind}"] = median_us(run_split)
                            assert not buf.download((len(segs),), np.uint32, st_at).any()
                            assert np.array_equal(out.download((H, W), np.uint16), mosaic), "the split path does not return the mosaic"
                            res[f"{bits}-bit split {kind}, to the difference plane"] = median_us(run_walk)
                            least = None
                            for r in list(range(1, 9)) + [16, 32, 64, 128]:
                                run_split(L.JpegSplitStruct(0, r))
                                lib.mi_device_synchronize(0)
                                if not (buf.download((len(segs),), np.uint32, st_at) & L.LJPEG_UNSYNCED).any():
                                    least = r
                                    break
                            rounds_info[f"{bits}-bit {kind}"] = {"enqueued": int(opt.max_rounds), "least_max_rounds_without_unsynced": least}
                        finally:
                            scratch.free()
                            plane.free()
                finally:
                    buf.free()
                sizes[f"{bits}-bit ljpeg {kind}"] = span.nbytes / ob
                del span, hs
            del host
        copy = res["copy of the output"][0]
        print(f"{H} x {W} ({H * W / 1e6:.1f} MP), {a.rounds} rounds of {a.reps}: median (min .. max) us", flush=True)
        for name, r in res.items():
            print(f"  {name:45s} {r[0]:10.1f} ({r[1]:10.1f} .. {r[2]:10.1f})   x copy {r[0] / copy:8.2f}   {H * W / r[0]:8.1f} Mpixel/s", flush=True)
        for name, f in sizes.items():
            print(f"  size of {name:30s} {f:6.3f} of the uint16 mosaic", flush=True)
        for name, f in rounds_info.items():
            print(f"  rounds of {name:30s} {f}", flush=True)
        if a.json:
            print(json.dumps({"height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "split_rounds": rounds_info,
                              "median_us": {k: round(v[0], 1) for k, v in res.items()},
                              "size_over_uint16_mosaic": {k: round(v, 4) for k, v in sizes.items()}}), flush=True)
    finally:
        out.free()
        src.free()
