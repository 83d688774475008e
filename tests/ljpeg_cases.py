"""A lossless-JPEG encoder, a compressed-DNG writer and the case table shared by test_ljpeg_restatement.py,
test_ljpeg_host.py, test_ljpeg_core_host.py (CPU) and test_gpu_ljpeg.py (GPU).

The encoder is written from the format's description (ITU-T T.81: process SOF3, Annex C codes, Annex H prediction), forwards,
with NumPy shifts for the neighbours, and never calls the restatement (tests/ljpeg_restatement.py) or the parser: it knows the
samples it stored, so what a reader must return is computed here from those samples.  All seven predictors, one or two
components, any precision; per segment an optimal table from the segment's own histogram (every tile gets a different one) or
a given one; FF 00 stuffing; padding with one-bits; an optional run of fill FF bytes in front of EOI.

Shapes, against the kernel's geometry (csrc/kernels_ljpeg.hpp: one segment per wave; the walker decodes batches of BATCH =
256 samples of one line out of a RING = 4096-byte ring staged in CHUNK = 256-byte steps; codes up to LUT_BITS = 10 bits come
from a lookup; predictors 2 to 7 keep the line above, up to MAX_LINE = 24576 columns); `paths` predicts what a case exercises.
"""
import functools
import heapq
import struct

import numpy as np

import dng_cases as DC

RING, CHUNK, BATCH, LUT_BITS, MAX_LINE = 4096, 256, 256, 10, 24576      # ljpeg:: of csrc/kernels_ljpeg.hpp

# the table of the two known answers: counts of the code lengths 1 .. 16, values in code order
KNOWN_TABLE = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
# a complete code with one code of every length 1 .. 15 and two of 16 bits (the second is sixteen one-bits): categories 0 .. 16
LONG_TABLE = ([1] * 15 + [2], list(range(17)))
# long codes for the SMALL categories: random data then needs the 16-bit codes all the time
LONG_TABLE_REVERSED = ([1] * 15 + [2], list(range(16, -1, -1)))


# ------------------------------------------------------------------------------------------------ the encoder
def differences(samples, ncomp, predictor, precision):
    """the differences (ints in [-32767, 32768]) of a segment's samples (rows x columns; column = x * ncomp + c)"""
    v = np.asarray(samples, np.int64)
    px = np.zeros_like(v)
    ra = np.zeros_like(v)
    ra[:, ncomp:] = v[:, :-ncomp]
    rb = np.zeros_like(v)
    rb[1:] = v[:-1]
    rc = np.zeros_like(v)
    rc[1:, ncomp:] = v[:-1, :-ncomp]
    px[...] = {1: ra, 2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1), 7: (ra + rb) >> 1}[predictor]
    px[0, :] = ra[0, :]
    px[1:, :ncomp] = rb[1:, :ncomp]
    px[0, :ncomp] = 1 << (precision - 1)
    d = (v - px) & 0xFFFF
    return np.where(d > 32768, d - 65536, d)


def category(d):
    return 0 if d == 0 else 16 if d == 32768 else int(abs(int(d))).bit_length()


def optimal_table(cats):
    """(counts, values) of a Huffman code for the categories that occur; 17 symbols never need more than 16 bits"""
    hist = {}
    for s in cats:
        hist[s] = hist.get(s, 0) + 1
    if len(hist) == 1:
        length = {next(iter(hist)): 1}
    else:
        heap = [(n, s, (s,)) for s, n in sorted(hist.items())]
        heapq.heapify(heap)
        length = dict.fromkeys(hist, 0)
        while len(heap) > 1:
            n1, t1, m1 = heapq.heappop(heap)
            n2, t2, m2 = heapq.heappop(heap)
            for s in m1 + m2:
                length[s] += 1
            heapq.heappush(heap, (n1 + n2, min(t1, t2), m1 + m2))
    assert max(length.values()) <= 16
    order = sorted(length, key=lambda s: (length[s], s))
    return [sum(1 for s in order if length[s] == n) for n in range(1, 17)], order


def code_of(table):
    """{category: (code, length)}: consecutive codes within a length, doubled from one length to the next"""
    counts, values = table
    out, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(counts[n - 1]):
            out[values[k]] = (code, n)
            code, k = code + 1, k + 1
        code *= 2
    return out


def entropy_bytes(diffs, ncomp, tables):
    """the stuffed entropy-coded data of a segment's differences, padded to a byte with one-bits; and the longest code used"""
    codes = [code_of(t) for t in tables]
    acc, nbits, longest = 0, 0, 0
    flat = diffs.reshape(-1)
    for i, d in enumerate(flat):
        d = int(d)
        s = category(d)
        code, n = codes[i % ncomp][s]
        longest = max(longest, n)
        acc, nbits = acc << n | code, nbits + n
        if 0 < s < 16:
            acc, nbits = acc << s | (d if d > 0 else d + (1 << s) - 1), nbits + s
    pad = -nbits % 8
    acc, nbits = acc << pad | (1 << pad) - 1, nbits + pad
    raw = acc.to_bytes(nbits // 8, "big") if nbits else b""
    return raw.replace(b"\xff", b"\xff\x00"), longest


def encode(samples, ncomp, predictor, precision, tables="optimal", fill_ff=0):
    """One JPEG stream for a segment's samples.  Returns (stream, info): info = {"scan_off": where the entropy-coded data
    starts in the stream, "data_bytes", "tables", "longest": the longest code used, "stuffed": FF 00 pairs in the data}."""
    samples = np.asarray(samples, np.int64)
    lines, w = samples.shape
    assert w % ncomp == 0
    d = differences(samples, ncomp, predictor, precision)
    if tables == "optimal":
        tables = [optimal_table([category(x) for x in d[:, c::ncomp].reshape(-1)]) for c in range(ncomp)]
    else:
        tables = [tables] * ncomp if isinstance(tables, tuple) else list(tables)
    data, longest = entropy_bytes(d, ncomp, tables)
    out = b"\xff\xd8"
    for c, (counts, values) in enumerate(tables):
        out += b"\xff\xc4" + struct.pack(">HB", 2 + 1 + 16 + len(values), c) + bytes(counts) + bytes(values)
    out += b"\xff\xc3" + struct.pack(">HBHHB", 8 + 3 * ncomp, precision, lines, w // ncomp, ncomp)
    out += b"".join(bytes([c + 1, 0x11, 0]) for c in range(ncomp))
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * ncomp, ncomp) + b"".join(bytes([c + 1, c << 4]) for c in range(ncomp))
    out += bytes([predictor, 0, 0])
    scan_off = len(out)
    out += data + b"\xff" * fill_ff + b"\xff\xd9"
    return out, {"scan_off": scan_off, "data_bytes": len(data), "tables": tables, "longest": longest, "stuffed": data.count(b"\xff\x00")}


# ------------------------------------------------------------------------------------------------ the DNG writer
def write_dng(path, stored, bits, ncomp=1, predictor=1, precision=None, tables="optimal", fill_ff=0, e="<", rows_per_strip=None,
              tile=None, order=None, gap=0, odd_start=False, pattern="RGGB", active_area=None, white=None, table=None, filler=None,
              mangle=None, extra=None, drop=(), black=None, neutral=None, matrices=None):
    """Write `stored` (H x W ints) as a DNG with Compression 7: every strip or tile one JPEG stream.  The geometry options are
    dng_cases.write_dng's.  mangle(k, stream, info) -> stream: what is written in place of segment k's stream.  Returns
    {"offsets": file offsets in grid order, "streams", "infos", "entries", "data_at": the file offset of the first segment byte}."""
    stored = np.asarray(stored, np.int64)
    h, w = stored.shape
    precision = bits if precision is None else precision
    sh, sw = tile if tile is not None else ((h if rows_per_strip is None else rows_per_strip), w)
    nsy, nsx = -(-h // sh), -(-w // sw)
    streams, infos = [], []
    for sy in range(nsy):
        for sx in range(nsx):
            block = stored[sy * sh:(sy + 1) * sh, sx * sw:(sx + 1) * sw]
            if tile is not None:        # edge tiles are stored at full size
                full = np.full((sh, sw), (1 << precision) - 1 if filler is None else filler, np.int64)
                full[:block.shape[0], :block.shape[1]] = block
                block = full
            s, info = encode(block, ncomp, predictor, precision, tables, fill_ff)
            if mangle is not None:
                s = mangle(len(streams), s, info)
            streams.append(s)
            infos.append(info)
    order = list(range(len(streams))) if order is None else list(order)
    assert sorted(order) == list(range(len(streams)))
    data, offsets = b"", [0] * len(streams)
    at = 8 + (1 if odd_start else 0)
    lead = b"\x5a" * (at - 8)
    for i, k in enumerate(order):
        offsets[k] = at + len(data)
        data += streams[k] + (b"\xa5" * gap if i + 1 < len(order) else b"")
    raw = {254: (4, [0]), 256: (4, [w]), 257: (4, [h]), 258: (3, [bits]), 259: (3, [7]), 262: (3, [32803]), 277: (3, [1]),
           284: (3, [1]), 33421: (3, [2, 2]), 33422: (1, list(DC.PATTERN_CODES[pattern])), 50710: (1, [0, 1, 2]), 50711: (3, [1])}
    if tile is not None:
        raw.update({322: (4, [sw]), 323: (4, [sh]), 324: (4, offsets), 325: (4, [len(s) for s in streams])})
    else:
        raw.update({273: (4, offsets), 278: (4, [sh]), 279: (4, [len(s) for s in streams])})
    if active_area is not None:
        raw[50829] = (4, list(active_area))
    if white is not None:
        raw[50717] = (4, [white])
    if table is not None:
        raw[50712] = (3, [int(v) for v in table])
    if black is not None:
        raw[50713] = (3, [1, 1])
        raw[50714] = (3, [int(b) for b in black])
    if neutral is not None:
        raw[50728] = (5, [DC.rational(v) for v in neutral])
    for k, (m, ill) in (matrices or {}).items():
        raw[50721 + k - 1] = (10, [DC.rational(v) for v in m])
        raw[50778 + k - 1] = (3, [ill])
    raw[50706] = (1, [1, 4, 0, 0])
    raw.update(extra or {})
    for tag in drop:
        raw.pop(tag, None)
    ifd_at = 8 + len(lead) + len(data)
    ifd_at += ifd_at & 1
    pad = b"\0" * (ifd_at - 8 - len(lead) - len(data))
    head = (b"II" if e == "<" else b"MM") + struct.pack(e + "HI", 42, ifd_at)
    with open(path, "wb") as fh:
        fh.write(head + lead + data + pad + DC._ifd_bytes(e, ifd_at, raw))
    return {"offsets": offsets, "streams": streams, "infos": infos, "entries": raw, "data_at": at}


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    """h x w samples of `precision` bits in a file of BitsPerSample `bits`; kw: write_dng's options"""

    def __init__(self, name, h, w, bits, ncomp=1, predictor=1, fill="random", precision=None, **kw):
        self.name, self.h, self.w, self.bits, self.ncomp, self.predictor, self.fill = name, h, w, bits, ncomp, predictor, fill
        self.precision = bits if precision is None else precision
        self.kw = kw

    def __repr__(self):
        return self.name

    @property
    def dtype(self):
        return np.dtype(np.uint8 if self.bits == 8 else np.uint16)

    @functools.lru_cache(maxsize=None)
    def stored(self):
        top = (1 << self.precision) - 1
        rng = np.random.default_rng([self.h, self.w, self.precision, self.ncomp, self.predictor, 43])
        if self.fill == "zeros":
            a = np.zeros((self.h, self.w), np.int64)
        elif self.fill == "ones":
            a = np.full((self.h, self.w), top, np.int64)
        elif self.fill == "mid":            # every difference 0 under predictor 1
            a = np.full((self.h, self.w), 1 << (self.precision - 1), np.int64)
        elif self.fill == "flip":           # every difference 32768 under predictor 1 at 16 bits: 0, 32768, 0, ... per component
            a = np.zeros((self.h, self.w), np.int64)
            x = np.arange(self.w) // self.ncomp
            a[:] = np.where(x % 2 == 0, 0, 32768)[None, :]
            a[1::2] ^= 32768                # (the first sample of a line is predicted from above)
        elif self.fill == "smooth":         # a ramp with a little noise: small categories, short codes
            yy, xx = np.mgrid[0:self.h, 0:self.w]
            a = np.clip((top // 4) + 3 * xx + 5 * yy + rng.integers(-6, 7, size=(self.h, self.w)), 0, top).astype(np.int64)
        else:
            a = rng.integers(0, top + 1, size=(self.h, self.w), dtype=np.int64)
            a.flat[0], a.flat[-1] = top, 0
        a.setflags(write=False)
        return a

    def white(self):
        return self.kw.get("white", (1 << self.bits) - 1)

    def shift(self):
        return max(0, 8 * self.dtype.itemsize - int(self.white()).bit_length())

    def crop(self):
        aa = self.kw.get("active_area")
        return (0, 0, self.h, self.w) if aa is None else (aa[0], aa[1], aa[2] - aa[0], aa[3] - aa[1])

    def segments(self):
        """(tiled, seg_h, seg_w)"""
        if self.kw.get("tile") is not None:
            return True, self.kw["tile"][0], self.kw["tile"][1]
        return False, self.kw.get("rows_per_strip") or self.h, self.w

    @functools.lru_cache(maxsize=None)
    def expected(self):
        """the mosaic a reader must return, from the stored samples themselves: crop, table (index clamped), shift"""
        top, left, ch, cw = self.crop()
        v = self.stored()[top:top + ch, left:left + cw]
        table = self.kw.get("table")
        if table is not None:
            v = np.asarray(table, np.int64)[np.minimum(v, len(table) - 1)]
        out = ((v << self.shift()) & int(np.iinfo(self.dtype).max)).astype(self.dtype)
        out.setflags(write=False)
        return out

    def write(self, path):
        return write_dng(path, self.stored(), self.bits, ncomp=self.ncomp, predictor=self.predictor, precision=self.precision, **self.kw)


CASES = [
    Case("12bit-2x2-one-strip", 2, 2, 12, ncomp=2),
    Case("12bit-2x4-one-strip", 2, 4, 12, ncomp=2),
    Case("12bit-5x17-nf1", 5, 17, 12, ncomp=1, predictor=4),
    Case("12bit-strips-of-1", 5, 18, 12, ncomp=2, rows_per_strip=1),
    Case("14bit-strips-of-3-short-last", 7, 18, 14, ncomp=2, predictor=2, rows_per_strip=3, order=(2, 0, 1), gap=5),
    Case("12bit-tiles-21x37-shuffled", 21, 37, 12, ncomp=2, tile=(16, 16), order=(5, 0, 3, 1, 4, 2), gap=7, odd_start=True, fill="smooth"),
    Case("14bit-tiles-21x37-p6", 21, 37, 14, ncomp=1, predictor=6, tile=(16, 16), filler=0x1234),
    Case("12bit-3x530", 3, 530, 12, ncomp=2),
    Case("12bit-3x530-p2", 3, 530, 12, ncomp=2, predictor=2, fill="smooth"),
    Case("12bit-3x530-p7-nf1", 3, 530, 12, ncomp=1, predictor=7, fill="smooth"),
    Case("16bit-64x130-random-long-stream", 64, 130, 16, ncomp=2),
    Case("16bit-flip-32768-all-stuffed", 4, 600, 16, ncomp=2, fill="flip", tables=LONG_TABLE),
    Case("16bit-flip-32768-all-stuffed-odd-start", 4, 600, 16, ncomp=2, fill="flip", tables=LONG_TABLE, odd_start=True),
    Case("16bit-long-codes", 6, 40, 16, ncomp=2, predictor=5, tables=LONG_TABLE_REVERSED, fill="smooth"),
    Case("12bit-single-code", 5, 18, 12, ncomp=2, fill="mid"),
    Case("12bit-known-table-fill-ff", 5, 18, 12, ncomp=2, tables=KNOWN_TABLE, fill="smooth", fill_ff=3),
    Case("12bit-table-short-shift-4", 5, 18, 12, ncomp=2, table=DC._ramp_table(3000)),
    Case("14bit-table-white-4095", 5, 17, 14, ncomp=1, predictor=3, table=DC._ramp_table(9000), white=4095),
    Case("12bit-zeros", 5, 18, 12, ncomp=2, fill="zeros"),
    Case("12bit-ones", 5, 18, 12, ncomp=2, fill="ones"),
    Case("16bit-ones-p4", 5, 18, 16, ncomp=2, predictor=4, fill="ones"),
    Case("12bit-be-file", 5, 18, 12, ncomp=2, e=">"),
    Case("8bit-5x18", 5, 18, 8, ncomp=2),
    Case("8bit-tiles-21x37-p5", 21, 37, 8, ncomp=1, predictor=5, tile=(16, 16)),
    Case("10bit-5x18", 5, 18, 10, ncomp=2, predictor=3),
    Case("16bit-file-12bit-precision", 5, 18, 16, ncomp=2, precision=12, white=4095),
    Case("12bit-2x24580-wider-than-the-line-buffer", 2, MAX_LINE + 4, 12, ncomp=2, fill="smooth"),
    Case("12bit-2x24576-p2-the-whole-line-buffer", 2, MAX_LINE, 12, ncomp=2, predictor=2),
    Case("12bit-2x24576-p6-the-whole-line-buffer", 2, MAX_LINE, 12, ncomp=1, predictor=6),
]
for _p in range(1, 8):
    for _nf in (1, 2):
        CASES.append(Case(f"12bit-7x{20 + _nf}-p{_p}-nf{_nf}", 7, 20 + _nf, 12, ncomp=_nf, predictor=_p,
                          fill="smooth" if _p % 2 else "random"))
for _py in (0, 1):
    for _px in (0, 1):
        CASES.append(Case(f"12bit-crop-{2 + _py}-{4 + _px}-strips", 24, 40, 12, ncomp=2, rows_per_strip=5, pattern="GRBG",
                          active_area=(2 + _py, 4 + _px, 21, 37), fill="smooth"))
        CASES.append(Case(f"14bit-crop-{2 + _py}-{4 + _px}-tiles-p{4 + _py + _px}", 24, 40, 14, ncomp=2, predictor=4 + _py + _px, tile=(16, 16),
                          active_area=(2 + _py, 4 + _px, 22, 39)))
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# short streams: the decoder's defined behaviour on data that ends early.  (case, the segment that is flagged, its flag)
def _cut(k, stream, info):
    return stream[:info["scan_off"] + info["data_bytes"] // 2] if k == 1 else stream


def _marker(k, stream, info):
    at = info["scan_off"] + info["data_bytes"] // 2
    return stream[:at] + b"\xff\xd9" + stream[at:] if k == 1 else stream


def _one_bit(k, stream, info):      # under the single-code table ("0": category 0) a one-bit leads no code
    at = info["scan_off"] + 2
    return stream[:at] + b"\x80" + stream[at + 1:] if k == 1 else stream


SHORT = [
    (Case("short-cut-mid-data", 9, 18, 12, ncomp=2, rows_per_strip=3, mangle=_cut), 1, 2),
    (Case("short-marker-mid-data", 9, 18, 12, ncomp=2, rows_per_strip=3, predictor=2, mangle=_marker), 1, 2),
    (Case("short-no-code-sparse-table", 27, 18, 12, ncomp=2, rows_per_strip=9, fill="mid", mangle=_one_bit), 1, 1),
]


# ------------------------------------------------------------------------------------------------ what a case exercises
PATHS = ("prefix-sum", "add-above", "serial", "one-component", "two-components", "carry", "partial-batch", "ring-wrap", "lut-miss",
         "stuffed", "stuffed-across-a-chunk", "no-line-buffer", "whole-line-buffer", "edge-tile", "crop", "table", "uint8", "several-segments")


def paths(case, info):
    """The kernel paths a case reaches (raw_ljpeg of csrc/kernels_ljpeg.hpp), from the geometry and the streams written
    (`info`: what write_dng returned; the span starts at the lowest segment offset):
      prefix-sum     predictor 1 (and every first line): the wave's per-component scan
      add-above      predictor 2 below the first line
      serial         predictors 3 to 7 below the first line: prediction stays with the walking lane
      one/two-components
      carry          a line of more than BATCH samples: the scan's carry and the walker's state cross batches
      partial-batch  a line whose length is no multiple of BATCH
      ring-wrap      a segment whose data is longer than the ring: staging wraps, RING // CHUNK steps do not fill it at once
      lut-miss       a code longer than LUT_BITS is used: the canonical search
      stuffed        the data holds FF 00
      stuffed-across-a-chunk   ... with the FF the last byte of a staging chunk and the 00 the first of the next
      no-line-buffer a segment wider than MAX_LINE
      whole-line-buffer   predictors 2 to 7 on a segment of exactly MAX_LINE columns: the largest LDS request, its last entry
      edge-tile      samples decoded and not written: outside the image
      crop, table, uint8, several-segments"""
    tiled, seg_h, seg_w = case.segments()
    seen = {"prefix-sum", "one-component" if case.ncomp == 1 else "two-components"}
    rows = seg_h if tiled else min(seg_h, case.h)
    if rows > 1 and case.predictor == 2:
        seen.add("add-above")
    if rows > 1 and case.predictor >= 3:
        seen.add("serial")
    if seg_w > BATCH:
        seen.add("carry")
    if seg_w % BATCH:
        seen.add("partial-batch")
    if seg_w > MAX_LINE:
        seen.add("no-line-buffer")
    if seg_w == MAX_LINE and rows > 1 and case.predictor >= 2:
        seen.add("whole-line-buffer")
    if tiled and (case.h % seg_h or case.w % seg_w):
        seen.add("edge-tile")
    if case.crop() != (0, 0, case.h, case.w):
        seen.add("crop")
    if case.kw.get("table") is not None:
        seen.add("table")
    if case.bits == 8:
        seen.add("uint8")
    if len(info["streams"]) > 1:
        seen.add("several-segments")
    lo = min(info["offsets"])
    for off, stream, i in zip(info["offsets"], info["streams"], info["infos"]):
        if i["data_bytes"] > RING:
            seen.add("ring-wrap")
        if i["longest"] > LUT_BITS:
            seen.add("lut-miss")
        if i["stuffed"]:
            seen.add("stuffed")
        scan = off - lo + i["scan_off"]             # in the span; staging starts at scan & ~3 and goes in steps of CHUNK
        data = stream[i["scan_off"]:i["scan_off"] + i["data_bytes"]]
        first = CHUNK - 1 - (scan - (scan & ~3))    # the data byte that is the last of the first chunk
        if any(data[j:j + 2] == b"\xff\x00" for j in range(first, len(data) - 1, CHUNK)):
            seen.add("stuffed-across-a-chunk")
    return seen


# ------------------------------------------------------------------------------------------------ the two known answers
KNOWN = [
    dict(precision=12, lines=2, x=2, ncomp=2, predictor=1, data=bytes.fromhex("1C92D73F41D3"),
         want=[[2048, 2050, 2047, 2055], [2040, 2050, 2303, 2049]]),
    dict(precision=12, lines=3, x=2, ncomp=2, predictor=1, data=bytes.fromhex("0FDFF0FDFF003F6E7FC18FFD803C6FFC003F"),
         want=[[2048, 2048, 2559, 2048], [2048, 2559, 2048, 3000], [100, 4095, 0, 2048]]),
]
