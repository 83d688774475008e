"""A small DNG writer and the case table shared by test_dng_host.py (CPU: the parser reads what was written, the cases mean
something) and test_gpu_dng.py (GPU: the kernel equals the restatement on them).

The writer is written from the format's description (TIFF 6.0 structure, the DNG tags by number, FillOrder 1 packing), not
from the parser: it lays the file out its own way -- sample data first, segments in any order with gaps, the IFDs behind them,
the raw IFD either IFD0 or a SubIFD behind a thumbnail IFD -- and knows the samples it stored, so what a reader must return is
computed here from those samples and never from packed bytes.

Shapes, against the kernel's geometry (unpack::TILE_H = 4 rows of 64 lanes, a lane owns a 16-byte window of its output row: 8
uint16 or 16 uint8 samples, aligned in memory; `paths` predicts what each case exercises):
  * widths 2, 3, 7, 8, 9, 17, 130 at 10, 12 and 14 bits, heights 2 and 5 (two workgroups down): under, on and over one window,
    rows that start off the 16-byte boundary (odd widths), the row tail; width 3 at 12 bits is a 5-byte row with half a byte of
    padding
  * 3 x 530 at 12 bits: the only way to a second workgroup ALONG a row (64 windows of 8 are 512 samples)
  * strips of 1, 3 and H rows; segments stored in shuffled order with gaps; a first segment at an odd file offset
  * 16 x 16 tiles on a 21 x 37 image: edge tiles, windows that cross a tile's edge
  * 16 bits in both byte orders, 8 bits
  * a crop with each parity of origin, on strips and on tiles
  * a linearisation table shorter than 2^bits with samples beyond it; shifts 0, 2, 4 (and 6 at 10 bits)
  * samples all zero and all ones"""
import functools
import struct

import numpy as np

XYZ_D65_MATRIX = (0.8, -0.2, -0.1, -0.4, 1.2, 0.2, -0.1, 0.3, 0.6)        # a made-up ColorMatrix (XYZ -> camera), row-major
OTHER_MATRIX = (0.9, -0.3, -0.05, -0.5, 1.3, 0.15, -0.05, 0.2, 0.7)
PATTERN_CODES = {"RGGB": (0, 1, 1, 2), "BGGR": (2, 1, 1, 0), "GRBG": (1, 0, 2, 1), "GBRG": (1, 2, 0, 1)}
_FMT = {1: "B", 3: "H", 4: "I", 7: "B", 12: "d"}
_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 7: 1, 10: 8, 12: 8}


# ------------------------------------------------------------------------------------------------ packing
def pack_rows(samples, bits, e):
    """the bytes of a segment: `samples` (rows x columns of ints below 2^bits), every row packed most significant bit first
    and padded with zero bits to a whole byte; 16 bits in the byte order `e`, 8 bits as they are"""
    a = np.asarray(samples, np.int64)
    if bits == 8:
        return a.astype(np.uint8).tobytes()
    if bits == 16:
        return a.astype(e + "u2").tobytes()
    rows = []
    for r in a:
        bit = ((r[:, None] >> np.arange(bits - 1, -1, -1)[None, :]) & 1).astype(np.uint8).reshape(-1)
        rows.append(np.packbits(np.concatenate([bit, np.zeros(-len(bit) % 8, np.uint8)])).tobytes())   # packbits: MSB first
    return b"".join(rows)


def _entry_bytes(e, typ, values):
    if typ == 2:
        return bytes(values)
    if typ in (5, 10):      # (numerator, denominator) pairs
        return b"".join(struct.pack(e + ("II" if typ == 5 else "ii"), n, d) for n, d in values)
    if typ == 7:
        return bytes(values)
    return struct.pack(e + _FMT[typ] * len(values), *values)


def _ifd_bytes(e, at, entries, next_ifd=0):
    """an IFD placed at file offset `at` with its out-of-line values right behind it.  entries: {tag: (type, values)}"""
    tags = sorted(entries)
    body_at = at + 2 + 12 * len(tags) + 4
    head, body = [struct.pack(e + "H", len(tags))], b""
    for tag in tags:
        typ, values = entries[tag]
        raw = _entry_bytes(e, typ, values)
        count = len(raw) // _SIZE[typ]
        if len(raw) <= 4:
            field = raw + b"\0" * (4 - len(raw))
        else:
            if (body_at + len(body)) & 1:
                body += b"\0"
            field = struct.pack(e + "I", body_at + len(body))
            body += raw
        head.append(struct.pack(e + "HHI", tag, typ, count) + field)
    return b"".join(head) + struct.pack(e + "I", next_ifd) + body


def rational(x, den=10000):
    return int(round(x * den)), den


def opcode_list(opcodes):
    """[(id, data)] as a DNG opcode list: big-endian whatever the file's order"""
    out = struct.pack(">I", len(opcodes))
    for oid, data in opcodes:
        out += struct.pack(">IIII", oid, 0x01030000, 0, len(data)) + data
    return out


def warp_rectilinear(planes, centre):
    data = struct.pack(">I", len(planes))
    for p in planes:
        data += struct.pack(">6d", *p)
    return 1, data + struct.pack(">2d", *centre)


def write_dng(path, stored, bits, e="<", rows_per_strip=None, tile=None, order=None, gap=0, odd_start=False, sub_ifd=False,
              pattern="RGGB", active_area=None, white=None, black=None, black_type=3, neutral=None, matrices=None, table=None,
              opcodes3=None, opcodes2=None, extra=None, drop=(), orientation=None, filler=None):
    """Write `stored` (H x W ints below 2^bits) as an uncompressed DNG.  Returns {"offsets": file offsets of the segments in
    grid order, "entries": the raw IFD's entries}.
    rows_per_strip / tile=(length, width): the segment geometry (default: one strip).  order: the order in which the segments
    lie in the file; gap: bytes of 0xA5 between them; odd_start: the first byte of sample data lies at an odd offset.
    sub_ifd: IFD0 is a thumbnail (NewSubFileType 1, RGB) and the raw IFD its only SubIFD; the colour tags stay in IFD0.
    matrices: {1: (matrix, illuminant), 2: ...}.  extra: further entries {tag: (type, values)} that replace what is written;
    drop: tags left out.
    filler: what the part of an edge tile outside the image holds (default: all ones)."""
    stored = np.asarray(stored, np.int64)
    h, w = stored.shape
    if tile is not None:
        sh, sw = tile
    else:
        sh, sw = (h if rows_per_strip is None else rows_per_strip), w
    nsy, nsx = -(-h // sh), -(-w // sw)
    segs = []
    for sy in range(nsy):
        for sx in range(nsx):
            block = stored[sy * sh:(sy + 1) * sh, sx * sw:(sx + 1) * sw]
            if tile is not None:        # edge tiles are stored at full size
                full = np.full((sh, sw), (1 << bits) - 1 if filler is None else filler, np.int64)
                full[:block.shape[0], :block.shape[1]] = block
                block = full
            segs.append(pack_rows(block, bits, e))
    order = list(range(len(segs))) if order is None else list(order)
    assert sorted(order) == list(range(len(segs)))
    data, offsets = b"", [0] * len(segs)
    at = 8 + (1 if odd_start else 0)
    lead = b"\x5a" * (at - 8)
    for i, k in enumerate(order):
        offsets[k] = at + len(data)
        data += segs[k] + (b"\xa5" * gap if i + 1 < len(order) else b"")
    raw = {254: (4, [0]), 256: (4, [w]), 257: (4, [h]), 258: (3, [bits]), 259: (3, [1]), 262: (3, [32803]), 277: (3, [1]),
           284: (3, [1]), 33421: (3, [2, 2]), 33422: (1, list(PATTERN_CODES[pattern])), 50710: (1, [0, 1, 2]), 50711: (3, [1])}
    if tile is not None:
        raw.update({322: (4, [sw]), 323: (4, [sh]), 324: (4, offsets), 325: (4, [len(s) for s in segs])})
    else:
        raw.update({273: (4, offsets), 278: (4, [sh]), 279: (4, [len(s) for s in segs])})
    if active_area is not None:
        raw[50829] = (4, list(active_area))
    if white is not None:
        raw[50717] = (4, [white])
    if black is not None:
        black = list(black)
        raw[50713] = (3, [2, 2] if len(black) == 4 else [1, 1])
        raw[50714] = (black_type, [rational(b) for b in black] if black_type == 5 else [int(b) for b in black])
    if table is not None:
        raw[50712] = (3, [int(v) for v in table])
    if opcodes3 is not None:
        raw[51022] = (7, opcode_list(opcodes3))
    if opcodes2 is not None:
        raw[51009] = (7, opcode_list(opcodes2))
    colour = {50706: (1, [1, 4, 0, 0])}
    if neutral is not None:
        colour[50728] = (5, [rational(v) for v in neutral])
    for k, (m, ill) in (matrices or {}).items():
        colour[50721 + k - 1] = (10, [rational(v) for v in m])
        colour[50778 + k - 1] = (3, [ill])
    if orientation is not None:
        colour[274] = (3, [orientation])
    for tag, ent in (extra or {}).items():
        (colour if tag in colour else raw)[tag] = ent
    for tag in drop:
        raw.pop(tag, None)
        colour.pop(tag, None)
    ifd_at = 8 + len(lead) + len(data)
    ifd_at += ifd_at & 1
    pad = b"\0" * (ifd_at - 8 - len(lead) - len(data))
    if not sub_ifd:
        blob = _ifd_bytes(e, ifd_at, {**colour, **raw})
    else:
        thumb = {254: (4, [1]), 256: (4, [1]), 257: (4, [1]), 258: (3, [8, 8, 8]), 259: (3, [1]), 262: (3, [2]), 273: (4, [8]),
                 277: (3, [3]), 278: (4, [1]), 279: (4, [3]), 330: (4, [0]), **colour}
        size0 = len(_ifd_bytes(e, ifd_at, thumb))
        sub_at = ifd_at + size0 + (size0 & 1)
        thumb[330] = (4, [sub_at])
        blob0 = _ifd_bytes(e, ifd_at, thumb)
        blob = blob0 + b"\0" * (sub_at - ifd_at - len(blob0)) + _ifd_bytes(e, sub_at, raw)
    head = (b"II" if e == "<" else b"MM") + struct.pack(e + "HI", 42, ifd_at)
    with open(path, "wb") as fh:
        fh.write(head + lead + data + pad + blob)
    return {"offsets": offsets, "entries": raw}


def write_truncated(path, stored, bits, cut=1, **kw):
    """a DNG whose sample data lies at the END of the file and is `cut` bytes short: the IFD comes first"""
    stored = np.asarray(stored, np.int64)
    h, w = stored.shape
    e = kw.get("e", "<")
    seg = pack_rows(stored, bits, e)
    raw = {254: (4, [0]), 256: (4, [w]), 257: (4, [h]), 258: (3, [bits]), 259: (3, [1]), 262: (3, [32803]), 277: (3, [1]),
           33421: (3, [2, 2]), 33422: (1, [0, 1, 1, 2]), 273: (4, [0]), 278: (4, [h]), 50706: (1, [1, 4, 0, 0])}
    if kw.get("byte_counts", False):
        raw[279] = (4, [len(seg) - cut])
    size = len(_ifd_bytes(e, 8, raw))
    raw[273] = (4, [8 + size])
    with open(path, "wb") as fh:
        fh.write((b"II" if e == "<" else b"MM") + struct.pack(e + "HI", 42, 8) + _ifd_bytes(e, 8, raw) +
                 (seg if kw.get("byte_counts", False) else seg[:len(seg) - cut]))


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, h, w, bits, fill="random", **kw):
        self.name, self.h, self.w, self.bits, self.fill, self.kw = name, h, w, bits, fill, kw

    def __repr__(self):
        return self.name

    @property
    def dtype(self):
        return np.dtype(np.uint8 if self.bits == 8 else np.uint16)

    @functools.lru_cache(maxsize=None)
    def stored(self):
        """the samples the file holds: H x W ints below 2^bits (seeded; full range)"""
        top = (1 << self.bits) - 1
        if self.fill == "zeros":
            a = np.zeros((self.h, self.w), np.int64)
        elif self.fill == "ones":
            a = np.full((self.h, self.w), top, np.int64)
        else:
            rng = np.random.default_rng([self.h, self.w, self.bits, 41])
            a = rng.integers(0, top + 1, size=(self.h, self.w), dtype=np.int64)
            a.flat[0], a.flat[-1] = top, 0
        a.setflags(write=False)
        return a

    def white(self):
        return self.kw.get("white", (1 << self.bits) - 1)

    def shift(self):
        """max(0, bits of the dtype - bit_length(WhiteLevel))"""
        return max(0, 8 * self.dtype.itemsize - int(self.white()).bit_length())

    def crop(self):
        """(top, left, height, width) of what a reader returns"""
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
        return write_dng(path, self.stored(), self.bits, **self.kw)


def _ramp_table(n, top=4095):
    """a linearisation table of n entries: a convex ramp ending at `top`"""
    return [int(round(top * (i / (n - 1)) ** 1.5)) for i in range(n)]


WARP = warp_rectilinear([(1.0, -0.05, 0.01, 0.0, 0.0, 0.0)], (0.5, 0.5))
WARP3 = warp_rectilinear([(1.01, 0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.99, 0.0, 0.0, 0.0, 0.0, 0.0)], (0.4, 0.6))
WARP_TANGENTIAL = warp_rectilinear([(1.0, 0.0, 0.0, 0.0, 0.001, 0.0)], (0.5, 0.5))
GAIN_MAP = (9, b"\0" * 76)

CASES = []
for _bits in (10, 12, 14):
    for _i, _w in enumerate((2, 3, 7, 8, 9, 17, 130)):
        CASES.append(Case(f"{_bits}bit-{2 if _i % 2 else 5}x{_w}", 2 if _i % 2 else 5, _w, _bits))
CASES += [
    Case("12bit-3x530-two-workgroups-along-a-row", 3, 530, 12),
    Case("12bit-strips-of-1", 5, 17, 12, rows_per_strip=1),
    Case("12bit-strips-of-3", 5, 17, 12, rows_per_strip=3),
    Case("14bit-strips-of-3-shuffled-gaps", 7, 9, 14, rows_per_strip=3, order=(2, 0, 1), gap=5),
    Case("10bit-strips-of-1-shuffled-gaps-odd-start", 5, 19, 10, rows_per_strip=1, order=(3, 1, 4, 0, 2), gap=3, odd_start=True),
    Case("12bit-odd-start", 5, 24, 12, odd_start=True),
    Case("16bit-odd-start-le", 5, 24, 16, odd_start=True),
    Case("12bit-tiles-21x37", 21, 37, 12, tile=(16, 16)),
    Case("10bit-tiles-21x37-shuffled", 21, 37, 10, tile=(16, 16), order=(5, 0, 3, 1, 4, 2), gap=7, odd_start=True),
    Case("14bit-tiles-21x37", 21, 37, 14, tile=(16, 16), filler=0x1234),
    Case("16bit-tiles-21x37-be", 21, 37, 16, tile=(16, 16), e=">"),
    Case("8bit-tiles-21x37", 21, 37, 8, tile=(16, 16)),
    Case("16bit-le-5x17", 5, 17, 16, e="<"),
    Case("16bit-be-5x17", 5, 17, 16, e=">"),
    Case("16bit-be-2x8", 2, 8, 16, e=">"),
    Case("8bit-5x17", 5, 17, 8),
    Case("8bit-2x16", 2, 16, 8),
    Case("8bit-5x47-odd-start", 5, 47, 8, odd_start=True, rows_per_strip=2),
    Case("12bit-be-file-5x17", 5, 17, 12, e=">"),
]
for _py in (0, 1):
    for _px in (0, 1):
        CASES.append(Case(f"12bit-crop-{2 + _py}-{4 + _px}-strips", 24, 40, 12, rows_per_strip=5, pattern="GRBG",
                          active_area=(2 + _py, 4 + _px, 21, 37)))
        CASES.append(Case(f"14bit-crop-{2 + _py}-{4 + _px}-tiles", 24, 40, 14, tile=(16, 16), pattern="RGGB",
                          active_area=(2 + _py, 4 + _px, 22, 39)))
CASES += [
    Case("10bit-crop-1-3-tiles", 20, 40, 10, tile=(16, 32), active_area=(1, 3, 19, 38)),
    Case("16bit-crop-1-1-be", 9, 21, 16, e=">", active_area=(1, 1, 8, 20)),
    Case("8bit-crop-1-3", 9, 40, 8, active_area=(1, 3, 8, 39)),
    Case("12bit-table-short", 5, 17, 12, table=_ramp_table(3000)),            # samples up to 4095 against 3000 entries
    Case("14bit-table-short-white-4095", 5, 17, 14, table=_ramp_table(9000), white=4095),
    Case("10bit-table-full", 2, 9, 10, table=_ramp_table(1024, 1023)),
    Case("16bit-shift-0", 2, 9, 16),
    Case("16bit-white-16383-shift-2", 5, 17, 16, white=16383),
    Case("12bit-shift-4", 5, 9, 12),
    Case("14bit-white-4000-shift-4", 5, 9, 14, white=4000),
    Case("8bit-white-63-shift-2", 2, 17, 8, white=63),
    Case("12bit-zeros", 5, 17, 12, fill="zeros"),
    Case("12bit-ones", 5, 17, 12, fill="ones"),
    Case("10bit-ones", 2, 9, 10, fill="ones"),
    Case("14bit-ones-tiles", 21, 37, 14, fill="ones", tile=(16, 16), filler=0),
    Case("16bit-ones-be", 2, 9, 16, fill="ones", e=">"),
    Case("14bit-zeros", 2, 9, 14, fill="zeros"),
    Case("12bit-sub-ifd-colour", 6, 10, 12, sub_ifd=True, pattern="GBRG", black=(256, 260, 258, 262), neutral=(0.5, 1.0, 0.625),
         matrices={1: (OTHER_MATRIX, 17), 2: (XYZ_D65_MATRIX, 21)}, opcodes3=[WARP], orientation=6),
    Case("14bit-colour-rational-black", 6, 10, 14, black=(1023.6,), black_type=5, neutral=(0.6, 1.0, 0.7),
         matrices={1: (XYZ_D65_MATRIX, 21), 2: (OTHER_MATRIX, 17)}, opcodes3=[GAIN_MAP, WARP3], opcodes2=[GAIN_MAP],
         extra={50715: (10, [rational(0.0)] * 10), 50727: (5, [rational(1.0)] * 3), 50719: (4, [0, 0]), 50720: (4, [10, 6])}),
    Case("12bit-colour-no-d65", 4, 6, 12, black=(64,), matrices={1: (OTHER_MATRIX, 17), 2: (XYZ_D65_MATRIX, 23)},
         opcodes3=[WARP_TANGENTIAL]),
    Case("12bit-colour-matrix1-only", 4, 6, 12, matrices={1: (OTHER_MATRIX, 17)}),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ what a case exercises
PATHS = ("whole", "partial", "tile-cross", "fifth dword", "unaligned", "bit offset", "span end")


def paths(case, offsets, span_bytes):
    """The kernel paths a case reaches (raw_unpack of csrc/kernels_unpack.hpp), from the geometry alone; `offsets`: the
    segment offsets rebased to the span.  The output is taken to start on a 16-byte boundary (a device allocation does).
      whole        a window of V samples inside one segment row: aligned dwords, funnel shift, one 16-byte store
      partial      a window that hangs over the row's start or end: sample by sample
      tile-cross   a window inside the row that crosses a tile's right edge: sample by sample
      fifth dword  a whole window whose bits reach into a fifth aligned dword
      unaligned    a whole window whose first byte is not on a dword boundary
      bit offset   a whole window whose first bit is not on a byte boundary
      span end     a whole window one of whose dwords reaches past the end of the span (put together from bytes)"""
    bits = case.bits
    item = case.dtype.itemsize
    V = 16 // item
    top, left, h, w = case.crop()
    _, seg_h, seg_w = case.segments()
    nsx = -(-case.w // seg_w)
    row_bytes = (seg_w * bits + 7) // 8
    seen = set()
    for y in range(h):
        off = (y * w * item % 16) // item
        for x0 in range(-off, w, V):
            if x0 < 0 or x0 + V > w:
                seen.add("partial")
                continue
            ys, xs = y + top, x0 + left
            xt = xs % seg_w
            if xt + V > seg_w:
                seen.add("tile-cross")
                continue
            seen.add("whole")
            k = (ys // seg_h) * nsx + xs // seg_w
            bit = xt * bits
            b = int(offsets[k]) + (ys % seg_h) * row_bytes + bit // 8
            sh = (b % 4) * 8 + bit % 8
            if b % 4:
                seen.add("unaligned")
            if bit % 8:
                seen.add("bit offset")
            if sh + V * bits > 128:
                seen.add("fifth dword")
            ndw = 5 if sh + V * bits > 128 else 4
            if (b - b % 4) + 4 * ndw > span_bytes:
                seen.add("span end")
    return seen
