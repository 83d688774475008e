#!/usr/bin/env python3
"""A fixed sequence of ten frames through the five raw push kinds of one handle -- plain, developed and calibrated mosaics,
packed spans and lossless-JPEG spans, twice over, the second time with site corrections set -- for a kernel trace:

    rocprofv3 --kernel-trace --stats -- python tools/push_trace.py

A change to the host side of the raw pushes (csrc/mosaic_host.hpp, the entry points of csrc/capi.hip) that keeps every
launch leaves the table of kernel names and call counts as it was.  Prints the number of frames pushed and a checksum of the
fused image."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

H, W, BITS, ROWS_PER_STRIP = 520, 776, 12, 64


def main():
    import ljpeg_encode
    from shinestacker_amd import _lib as L
    from shinestacker_amd import dng
    from shinestacker_amd.demosaic import Calibration, Cfa, Develop
    L.require_device()
    rng = np.random.default_rng(11)
    cfa = Cfa("RGGB", black=1024, gains=[1.8, 1.0, 1.0, 1.4])
    y, x = np.mgrid[0:H, 0:W]
    stored = [np.clip(2048 + 1500 * np.sin(x / (9.0 + k)) * np.cos(y / 13.0) + rng.integers(-200, 200, size=(H, W)), 0, 4095).astype(np.uint16)
              for k in range(10)]
    mosaics = [(v << (16 - BITS)).astype(np.uint16) for v in stored]
    rowb = W * BITS // 8
    offsets = np.arange(-(-H // ROWS_PER_STRIP), dtype=np.uint32) * np.uint32(ROWS_PER_STRIP * rowb)
    layout = dng.RawLayout(BITS, False, H, W, False, ROWS_PER_STRIP, W, offsets, shift=16 - BITS)

    def packed(v):      # two 12-bit samples are three bytes
        a, b = v[:, 0::2], v[:, 1::2]
        span = np.stack([a >> 4, (a & 15) << 4 | b >> 8, b & 255], axis=2).astype(np.uint8).reshape(-1)
        return dng.DngFrame("<memory>", layout, span, cfa, None, None, 1, ())

    def ljpeg(v):
        span, segs = ljpeg_encode.encode_frame(v, BITS, 128, 256, True)
        lay = dng.RawLayout(BITS, False, H, W, True, 128, 256, np.zeros(len(segs), np.uint32), shift=16 - BITS, compression=7, segments=segs)
        return dng.DngFrame("<memory>", lay, span, cfa, None, None, 1, ())

    sites = np.stack([rng.integers(0, H, 500), rng.integers(0, W, 500)], axis=1)
    corrections = dng.SiteCorrections(black_h=np.arange(W) % 3 - 1, black_v=1 - np.arange(H) % 3,
                                      gains=dng.GainMap(rng.uniform(0.8, 1.6, size=(13, 17)), spacing=(1.0 / 12, 1.0 / 16)),
                                      bad_sites=np.flatnonzero(rng.random(H * W) < 0.001))
    with Develop(matrix=[[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [0.05, -0.55, 1.5]], tone="srgb", defects=sites) as dv, \
            Calibration(dark=rng.integers(0, 512, size=(H, W)).astype(np.uint16), flat=np.full((H, W), 40000, np.uint16)) as cb, \
            L.Stack(H, W, in_dtype=np.uint16, batch_frames=4) as st:
        for k in range(10):
            if k == 5:
                st.set_site_correction(corrections)
            kind = k % 5
            if kind == 0:
                st.push_mosaic(mosaics[k], cfa)
            elif kind == 1:
                st.push_mosaic(mosaics[k], cfa, develop=dv)
            elif kind == 2:
                st.push_mosaic(mosaics[k], cfa, develop=dv, calibration=cb)
            elif kind == 3:
                st.push_packed(packed(stored[k]), develop=dv)
            else:
                st.push_packed(ljpeg(stored[k]), calibration=cb)
        assert st.ljpeg_status() == 0
        pushed = st.frames_pushed
        out = st.finish()
    corrections.close()
    print(f"frames pushed: {pushed}; crc32 of the fused image: {zlib.crc32(out.tobytes()):08x}")


if __name__ == "__main__":
    main()
