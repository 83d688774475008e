"""A NumPy lossless-JPEG encoder for the timing tools (ljpeg_time.py, config5.py --ljpeg): whole frames of tens of megapixels in
seconds, where the plain encoder of tests/ljpeg_cases.py takes minutes.  Predictor 1, one or two components, an optimal
Huffman table per segment from the segment's own histogram, FF 00 stuffing, one-bit padding: what a converter writes.  Both
tools decode what this wrote on the device and compare it with the mosaic they started from, so a mistake here cannot go
unnoticed.

`scene(h, w, bits, seed)`: the test content -- a smooth field (a diagonal ramp plus four broad Gaussian blobs, 5 % to 60 % of
full scale) with sensor-like noise: shot noise of standard deviation sqrt(signal * 2^(bits - 12)) and read noise of 2^(bits - 12)
* 1.5 counts, on a 2 x 2 colour cell whose four sites see 0.6, 1.0, 1.0 and 0.45 of the field.  Random samples would not
compress at all and a noiseless ramp would compress to nothing: both would misstate sizes and times."""
import heapq
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

POW2 = 1 << np.arange(16, dtype=np.int64)          # category s = how many of 1, 2, 4, ... are <= |d|


def scene(h, w, bits, seed=0):
    rng = np.random.default_rng([h, w, bits, seed])
    yy = np.linspace(0.0, 1.0, h, dtype=np.float32)[:, None]
    xx = np.linspace(0.0, 1.0, w, dtype=np.float32)[None, :]
    f = 0.05 + 0.15 * (0.6 * xx + 0.4 * yy)
    for cy, cx, r, a in ((0.3, 0.3, 0.2, 0.25), (0.7, 0.6, 0.3, 0.2), (0.5, 0.85, 0.12, 0.15), (0.8, 0.15, 0.15, 0.1)):
        f = f + a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    cell = np.array([[0.6, 1.0], [1.0, 0.45]], np.float32)
    f = f * np.tile(cell, (h // 2 + 1, w // 2 + 1))[:h, :w]
    full = float((1 << bits) - 1)
    k = 2.0 ** (bits - 12)
    sig = f * full
    noisy = sig + rng.standard_normal((h, w), dtype=np.float32) * np.sqrt(sig * k + (1.5 * k) ** 2)
    return np.clip(np.rint(noisy), 0, full).astype(np.uint16)


def _table(hist):
    """(counts, values, code[17], length[17]) of an optimal code for the categories with hist > 0"""
    syms = [s for s in range(17) if hist[s]]
    length = dict.fromkeys(syms, 1 if len(syms) == 1 else 0)
    heap = [(int(hist[s]), s, (s,)) for s in syms]
    heapq.heapify(heap)
    while len(heap) > 1:
        n1, t1, m1 = heapq.heappop(heap)
        n2, t2, m2 = heapq.heappop(heap)
        for s in m1 + m2:
            length[s] += 1
        heapq.heappush(heap, (n1 + n2, min(t1, t2), m1 + m2))
    order = sorted(syms, key=lambda s: (length[s], s))
    counts = [sum(1 for s in order if length[s] == n) for n in range(1, 17)]
    code, lens = np.zeros(17, np.int64), np.zeros(17, np.int64)
    c, k = 0, 0
    for n in range(1, 17):
        for _ in range(counts[n - 1]):
            code[order[k]], lens[order[k]] = c, n
            c, k = c + 1, k + 1
        c <<= 1
    return counts, order, code, lens


def encode_segment(block, ncomp, precision):
    """one JPEG stream (bytes) for a segment's samples (rows x columns, column = x * ncomp + c), predictor 1; and the offset of
    its entropy-coded data"""
    v = block.astype(np.int64)
    lines, w = v.shape
    px = np.empty_like(v)
    px[:, ncomp:] = v[:, :-ncomp]
    px[1:, :ncomp] = v[:-1, :ncomp]
    px[0, :ncomp] = 1 << (precision - 1)
    d = (v - px) & 0xFFFF
    d = np.where(d > 32768, d - 65536, d).reshape(-1)
    s = np.searchsorted(POW2, np.abs(d), side="right")          # 0 for 0, 16 for 32768
    extra = np.where(d >= 0, d, d + (1 << s) - 1)
    nx = np.where(s == 16, 0, s)
    comp = np.arange(d.size) % ncomp
    val, nb = np.zeros(d.size, np.int64), np.zeros(d.size, np.int64)
    tables = []
    for c in range(ncomp):
        m = comp == c
        counts, values, code, lens = _table(np.bincount(s[m], minlength=17))
        tables.append((counts, values))
        val[m] = code[s[m]] << nx[m] | np.where(s[m] == 16, 0, extra[m])
        nb[m] = lens[s[m]] + nx[m]
    bits = np.unpackbits(val.astype(">u4").view(np.uint8).reshape(-1, 4), axis=1)       # 32 bits a sample, the code's last
    stream = bits[np.arange(32)[None, :] >= (32 - nb)[:, None]]                         # ... nb of them, in order
    stream = np.concatenate([stream, np.ones(-stream.size % 8, np.uint8)])
    data = np.packbits(stream).tobytes().replace(b"\xff", b"\xff\x00")
    out = b"\xff\xd8"
    for c, (counts, values) in enumerate(tables):
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(values), c) + bytes(counts) + bytes(values)
    out += b"\xff\xc3" + struct.pack(">HBHHB", 8 + 3 * ncomp, precision, lines, w // ncomp, ncomp)
    out += b"".join(bytes([c + 1, 0x11, 0]) for c in range(ncomp))
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * ncomp, ncomp) + b"".join(bytes([c + 1, c << 4]) for c in range(ncomp)) + bytes([1, 0, 0])
    return out + data + b"\xff\xd9", len(out), tables


def encode_frame(mosaic, bits, seg_h, seg_w, tiled, ncomp=2, threads=16):
    """(span: uint8 array of the segments' streams back to back, each starting on a multiple of 4; the mi_ljpeg_seg_t records,
    LJPEG_SEG_DTYPE) of a whole H x W mosaic of `bits`-bit samples in strips or tiles (edge tiles padded with their last
    column and row)"""
    from shinestacker_amd import _lib
    h, w = mosaic.shape
    nsy, nsx = -(-h // seg_h), -(-w // seg_w)

    def one(k):
        sy, sx = divmod(k, nsx)
        block = mosaic[sy * seg_h:(sy + 1) * seg_h, sx * seg_w:(sx + 1) * seg_w]
        if tiled and block.shape != (seg_h, seg_w):
            block = np.pad(block, ((0, seg_h - block.shape[0]), (0, seg_w - block.shape[1])), mode="edge")
        return encode_segment(block, ncomp, bits)
    with ThreadPoolExecutor(threads) as pool:
        done = list(pool.map(one, range(nsy * nsx)))
    segs = np.zeros(len(done), _lib.LJPEG_SEG3_DTYPE if ncomp == 3 else _lib.LJPEG_SEG_DTYPE)     # (mi_ljpeg_seg3_t: three tables)
    parts, at = [], 0
    for k, (stream, scan, tables) in enumerate(done):
        rows = seg_h if tiled else min(seg_h, h - (k // nsx) * seg_h)
        r = segs[k]
        r["scan_off"], r["scan_bytes"], r["x"], r["y"] = at + scan, len(stream) - scan, seg_w // ncomp, rows
        r["ncomp"], r["predictor"], r["precision"] = ncomp, 1, bits
        for c, (counts, values) in enumerate(tables):
            r["counts"][c, :] = counts
            r["values"][c, :len(values)] = values
        pad = -len(stream) % 4
        parts.append(stream + b"\0" * pad)
        at += len(stream) + pad
    return np.frombuffer(b"".join(parts), np.uint8), segs
