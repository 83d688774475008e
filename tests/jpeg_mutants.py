"""Seeded corrupt baseline-JPEG files: the corpus shared by test_jpeg_mutants_host.py, test_jpeg_core_host.py,
test_jpeg_split_core_host.py (CPU) and test_gpu_jpeg_mutants.py (GPU).  The shape of tests/dng_mutants.py.

The BASES are the writer's files (jpeg_cases.CASES, the hand-made symbol cases and SHORT; jpeg_split_cases.PLAIN and LONG,
the files without a restart interval and with one above jpeg.MAX_DRI) and, where Pillow imports, a handful of Pillow's
(PILLOW picks them from jpeg_cases.pillow_files()).  Every test file is a base with one thing changed:

    blind mutators      one bit flipped; one byte set to 00 / 01 / 7F / 80 / FF; the file cut at a random length and at every
                        structure boundary (each marker segment's first and last byte, the first and last byte of the scan,
                        each RSTn)
    structure-aware     this module walks the file's own markers (`Structure`) and sets every segment length, DQT's Pq, Tq
                        and single entries, DHT's Tc, Th, counts (one that oversubscribes the code space among them;
                        `dht-move` moves one code to another length, which keeps the table's size) and values (a DC category
                        above 15, AC values over the whole byte), SOF0's precision, Y, X, Nf and each component's id, H, V
                        and Tq, the DRI value (0, 1, 8192, 8193 and 65535 among them), SOS's Ns, Cs, Td, Ta, Ss, Se, Ah and
                        Al, the JFIF and Adobe bodies (the transform byte among them), the Exif orientation entry's type,
                        count and value, its IFD's offset and entry count -- a field to each of 0, 1, the field's largest
                        value and its own value +- 1; one segment removed; one duplicated (a second SOF0 of another size, a
                        second DRI, a DHT repeated with other contents); and the scan data: a bit, a marker written over two
                        bytes (RSTn out of order, EOI early, a foreign marker), FF as the last byte, sixteen one-bits, FF FF,
                        the scan less its last k bytes

A mutant is its bytes and a one-line recipe (base, kind, seed, position, value): `position` is the file offset of the first
byte changed (the new length of a cut), `value` the new bytes in hex.  Everything is seeded NumPy; nothing here touches a device.

`parse(b, m)` gives a mutant to jpeg.read at split=None, "needed" and "always" and keeps what came back for each (a frame,
or the exception) with the time the three parses took; `outcomes()` does so for every mutant once.  `restated(outcome)` is
jpeg_restatement.parse, then walk (files read with restart intervals) and jpeg_split_restatement.walk_split (every file),
computed once per distinct (headers, scan bytes) -- most accepted mutants changed a byte no coefficient depends on -- and
render of either on demand.  `device_selection()` picks what the GPU file runs.

An accepted mutant may describe a much larger picture than its base (Y set to 65535 in a file without restart intervals):
one of more than MAX_SAMPLES = 65 536 samples takes part in the parser tests only (`Outcome.restate` is False), as the
24576-wide DNG cases do.  The largest base, 129 x 150, has 19 350.

Sizes with Pillow (139 bases and 22 996 mutants without it): 145 bases, 23 912 mutants; jpeg.read accepts 5 139 at split=None
and 9 153 at "needed" and at "always"; 9 079 of those are of at most MAX_SAMPLES samples, 7 083 of them distinct.  Per (mode,
with or without restart intervals) the distinct accepted mutants hold 70 to 200 of status 0 with other coefficients, 100 to
310 NOCODE, 85 to 250 OVERRUN, 22 to 100 RUN, 11 to 34 `dht-move` that still decode, 55 to 148 changed quantisation entries
and 34 to 81 markers in the middle of an interval (test_jpeg_mutants_host.py asserts each cell, rounded down).  Parsing takes
19 s on a shared CPU machine and 9 s on the GPU machine's host, restating every distinct accepted mutant 35 to 45 s;
`device_selection()` restates at most CLASS_TRIES candidates a base and takes 12 s on the GPU machine's host, parsing included.
"""
import atexit
import functools
import hashlib
import os
import shutil
import struct
import tempfile
import time

import numpy as np

import jpeg_cases as JC
import jpeg_restatement as R
import jpeg_split_cases as SC
import jpeg_split_restatement as S
from dng_mutants import BYTE_VALUES, DEVICE_LIMIT, Mutant, _cut, _field_values, _no_collection, _patched
from shinestacker_amd import jpeg

NOCODE, OVERRUN, RUN = R.NOCODE, R.OVERRUN, R.RUN
SPLITS = (None, "needed", "always")
MAX_SAMPLES = 1 << 16   # width x height above which an accepted mutant is parsed and not restated
HEAVY = 5000            # samples: a base with more gets the smaller blind and scan counts (its restatement takes longer)
BLIND = {False: (8, 8, 4), True: (3, 3, 2)}       # heavy -> (bit flips, byte sets, random cuts)
SCAN_BITS = {False: 8, True: 3}
# bases whose every header field is mutated; the others get a seeded sample of STRUCT_SAMPLE field mutants
FULL_STRUCTURE = ("cases/17x33-420-row", "cases/37x53-444-dri3", "cases/37x53-422-dri3", "cases/8x9-grey-row", "cases/exif-orientation",
                  "cases/adobe-ycc", "plain/17x33-420", "plain/37x53-444", "plain/16x16-422", "plain/8x9-grey", "long/17x33-420-dri8193")
STRUCT_SAMPLE = 30
PILLOW = ("pil-17x33-444-q90-restart_marker_rows", "pil-17x33-422-q30-restart_marker_blocks", "pil-37x53-420-q90-restart_marker_blocks",
          "pil-31x15-grey-q100-restart_marker_rows", "pil-37x53-420-q100-restart_marker_blocks-optimize", "pil-narrow-5x3-422")
MODES = ("444", "422", "420", "grey")


# ------------------------------------------------------------------------------------------------ the bases
class Base:
    """one file: `data` its bytes, `mode` its sampling ("444", "422", "420", "grey"), `dri` its restart interval (0: none)"""

    def __init__(self, name, data):
        self.name, self.data, self.index = name, bytes(data), -1
        h = R.parse(self.data)
        self.dri, self.samples = h["dri"], h["width"] * h["height"]
        self.mode = "grey" if h["ncomp"] == 1 else {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[(h["hmax"], h["vmax"])]

    def __repr__(self):
        return self.name

    @property
    def heavy(self):
        return self.samples > HEAVY

    @property
    def serial(self):
        """jpeg.read takes the file at split=None: it has a restart interval of at most jpeg.MAX_DRI MCUs"""
        return 1 <= self.dri <= jpeg.MAX_DRI

    @functools.lru_cache(maxsize=None)
    def structure(self):
        return Structure(self.data)


@functools.lru_cache(maxsize=None)
def workdir():
    d = tempfile.mkdtemp(prefix="jpeg-mutants-")
    atexit.register(shutil.rmtree, d, True)
    return d


@functools.lru_cache(maxsize=None)
def bases():
    out = [Base("cases/" + c.name, c.data()) for c in JC.CASES + [s[0] for s in JC.SHORT]]
    out += [Base("plain/" + c.name, c.data()) for c in SC.PLAIN]
    out += [Base("long/" + c.name, c.data()) for c in SC.LONG]
    pil = dict(JC.pillow_files())       # (empty without Pillow: those bases are left out, not failed)
    out += [Base("pillow/" + name, pil[name]) for name in PILLOW if name in pil]
    assert len({b.name for b in out}) == len(out)
    for i, b in enumerate(out):
        b.index = i
    return tuple(out)


def base(name):
    return next(b for b in bases() if b.name == name)


# ------------------------------------------------------------------------------------------------ where the files keep things
class Structure:
    """A clean file, walked: `segments` [(marker, offset of its FF, length field)] up to and with SOS, `scan` the scan's first
    byte, `end` the offset of EOI's FF, `rst` the offsets of the RSTn markers' FFs, `boundaries` the sorted offsets at which a
    cut is tried"""

    def __init__(self, data):
        at, self.segments = 2, []
        while True:
            assert data[at] == 0xFF, at
            m, n = data[at + 1], data[at + 2] << 8 | data[at + 3]
            self.segments.append((m, at, n))
            at += 2 + n
            if m == 0xDA:
                break
        self.scan = at
        self.rst, i = [], at
        while not (data[i] == 0xFF and data[i + 1] == 0xD9):
            if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7:
                self.rst.append(i)
            i += 2 if data[i] == 0xFF else 1
        self.end = i
        bounds = {2, self.scan, self.scan + 1, self.end - 1, self.end, self.end + 1}
        for _, a, n in self.segments:       # in front of the segment, behind its marker, behind its length, its last byte
            bounds |= {a, a + 2, a + 4, a + 1 + n}
        for k, r in enumerate(self.rst):    # between the FF and the Dn of every RSTn; in front of and behind the first three
            bounds |= {r + 1} | ({r, r + 2} if k < 3 else set())
        self.boundaries = sorted(x for x in bounds if 0 <= x < len(data))

    def first(self, marker):
        return next(((a, n) for m, a, n in self.segments if m == marker), None)

    def intervals(self):
        """[(first byte, byte behind the last)] of the scan's restart intervals"""
        starts = [self.scan] + [r + 2 for r in self.rst]
        return list(zip(starts, self.rst + [self.end]))


# ------------------------------------------------------------------------------------------------ the mutants
def _field(b, kind, pos, size, out, values=None):
    """`out` += the mutants of the `size`-byte big-endian field at `pos`"""
    fmt = ">" + {1: "B", 2: "H", 4: "I"}[size]
    own = struct.unpack_from(fmt, b.data, pos)[0]
    for v in (_field_values(own, size) if values is None else [v for v in dict.fromkeys(values) if v != own]):
        out.append(_patched(b, kind, v, [(pos, struct.pack(fmt, v))]))


def _nibble(b, kind, pos, high, out):
    """... of the high or low half of the byte at `pos`: 0, 1, 15 and its own value +- 1"""
    byte = b.data[pos]
    own = byte >> 4 if high else byte & 15
    for v in dict.fromkeys((0, 1, 15, (own - 1) & 15, (own + 1) & 15)):
        if v != own:
            out.append(_patched(b, kind, v, [(pos, bytes([(v << 4) | (byte & 15) if high else (byte & 0xF0) | v]))]))


def _spliced(b, kind, seed, at, remove, insert):
    """the base with `remove` bytes at `at` replaced by `insert`: the file's length changes"""
    data = b.data[:at] + bytes(insert) + b.data[at + remove:]
    return Mutant(b, kind, seed, at, f"-{remove} +{bytes(insert).hex()}", data, False)


def blind_mutants(b):
    rng = np.random.default_rng([b.index, 201])
    nbit, nbyte, ncut = BLIND[b.heavy]
    n, out = len(b.data), []
    for s in range(nbit):
        pos, bit = int(rng.integers(n)), int(rng.integers(8))
        out.append(_patched(b, "bit", s, [(pos, bytes([b.data[pos] ^ 1 << bit]))], True))
    for s in range(nbyte):
        pos, v = int(rng.integers(n)), BYTE_VALUES[int(rng.integers(len(BYTE_VALUES)))]
        out.append(_patched(b, "byte", s, [(pos, bytes([v]))], True))
    for s in range(ncut):
        out.append(_cut(b, "cut", s, int(rng.integers(n))))
    for s, at in enumerate(b.structure().boundaries):
        out.append(_cut(b, "cut-boundary", s, at))
    return [m for m in out if m is not None]


def _dht_tables(data, at, n):
    """[(offset of the Tc/Th byte, counts)] of the tables of one DHT segment"""
    q, out = at + 4, []
    while q + 17 <= at + 2 + n:
        counts = list(data[q + 1:q + 17])
        out.append((q, counts))
        q += 17 + sum(counts)
    return out


def header_mutants(b):
    """every field of every marker segment in front of the scan"""
    st, out = b.structure(), []
    rng = np.random.default_rng([b.index, 203])
    d = b.data
    for m, at, n in st.segments:
        _field(b, f"length-{m:02x}", at + 2, 2, out)
        body = at + 4
        if m == 0xDB:
            q = body
            while q + 65 <= at + 2 + n:
                _nibble(b, "dqt-pq", q, True, out)
                _nibble(b, "dqt-tq", q, False, out)
                for k in sorted({0, 63, int(rng.integers(64)), int(rng.integers(64))}):
                    _field(b, "dqt-entry", q + 1 + k, 1, out)
                q += 65
        elif m == 0xC4:
            for q, counts in _dht_tables(d, at, n):
                nval, dc = sum(counts), d[q] >> 4 == 0
                used = [i for i, c in enumerate(counts) if c]
                _nibble(b, "dht-tc", q, True, out)
                _nibble(b, "dht-th", q, False, out)
                out.append(_patched(b, "dht-count", 0, [(q + 1, bytes([3]))]))                  # three codes of one bit
                for s in range(2):
                    _field(b, "dht-count", q + 1 + int(rng.integers(16)), 1, out)
                for s in range(8):      # one code from a length that has one to another length: the table keeps its size
                    a, c = used[int(rng.integers(len(used)))], int(rng.integers(16))
                    if a != c and counts[c] < 255:
                        out.append(_patched(b, "dht-move", s, [(q + 1 + a, bytes([counts[a] - 1])), (q + 1 + c, bytes([counts[c] + 1]))]))
                values = (0, 15, 16, 17, 255, int(rng.integers(18, 255))) if dc else (0x00, 0xF0, 0xFF, 0x0F, int(rng.integers(256)), int(rng.integers(256)))
                for s, v in enumerate(values):
                    out.append(_patched(b, "dht-value", s, [(q + 17 + int(rng.integers(nval)), bytes([v]))]))
        elif m in (0xC0, 0xC1):
            _field(b, "sof-precision", body, 1, out)
            _field(b, "sof-y", body + 1, 2, out)
            _field(b, "sof-x", body + 3, 2, out)
            _field(b, "sof-nf", body + 5, 1, out)
            for c in range(d[body + 5]):
                _field(b, "sof-id", body + 6 + 3 * c, 1, out)
                _nibble(b, "sof-h", body + 7 + 3 * c, True, out)
                _nibble(b, "sof-v", body + 7 + 3 * c, False, out)
                _field(b, "sof-tq", body + 8 + 3 * c, 1, out)
        elif m == 0xDD:
            own = d[body] << 8 | d[body + 1]
            _field(b, "dri", body, 2, out, values=(0, 1, 8192, 8193, 65535, (own - 1) & 0xFFFF, (own + 1) & 0xFFFF))
        elif m == 0xDA:
            ns = d[body]
            _field(b, "sos-ns", body, 1, out)
            for c in range(ns):
                _field(b, "sos-cs", body + 1 + 2 * c, 1, out)
                _nibble(b, "sos-td", body + 2 + 2 * c, True, out)
                _nibble(b, "sos-ta", body + 2 + 2 * c, False, out)
            _field(b, "sos-ss", body + 1 + 2 * ns, 1, out)
            _field(b, "sos-se", body + 2 + 2 * ns, 1, out)
            _nibble(b, "sos-ah", body + 3 + 2 * ns, True, out)
            _nibble(b, "sos-al", body + 3 + 2 * ns, False, out)
        elif m == 0xE0:
            for k in range(min(n - 2, 14)):         # the identifier, the version, the units and densities, the thumbnail's size
                _field(b, "jfif-body", body + k, 1, out, values=(0, 0xFF) if k < 7 else (0xFF,))
        elif m == 0xEE:
            for k in range(n - 3):
                _field(b, "adobe-body", body + k, 1, out, values=(0, 0xFF))
            _field(b, "adobe-transform", body + n - 3, 1, out, values=(0, 1, 2, 3, 0xFF))
        elif m == 0xE1 and d[body:body + 6] == b"Exif\0\0":
            tiff = body + 6
            e = "<" if d[tiff:tiff + 2] == b"II" else ">"
            ifd = tiff + struct.unpack_from(e + "I", d, tiff + 4)[0]
            fmt = {1: e + "B", 2: e + "H", 4: e + "I"}

            def put(kind, pos, size):
                own = struct.unpack_from(fmt[size], d, pos)[0]
                for v in _field_values(own, size):
                    out.append(_patched(b, kind, v, [(pos, struct.pack(fmt[size], v))]))
            out.append(_patched(b, "exif-order", 0, [(tiff, b"MM")]))
            put("exif-ifd-offset", tiff + 4, 4)
            put("exif-entries", ifd, 2)
            for i in range(struct.unpack_from(e + "H", d, ifd)[0]):
                ent = ifd + 2 + 12 * i
                if struct.unpack_from(e + "H", d, ent)[0] == 0x0112:
                    put("exif-tag", ent, 2)
                    put("exif-type", ent + 2, 2)
                    put("exif-count", ent + 4, 4)
                    put("exif-value", ent + 8, 2)
                    for v in range(2, 10):
                        out.append(_patched(b, "exif-value", v, [(ent + 8, struct.pack(fmt[2], v))]))
                    put("exif-value-offset", ent + 8, 4)
    return [m for m in out if m is not None]


def segment_mutants(b):
    """one marker segment removed; one duplicated with other contents"""
    st, out, d = b.structure(), [], b.data
    for s, (m, at, n) in enumerate(st.segments):
        out.append(_spliced(b, f"remove-{m:02x}", s, at, 2 + n, b""))
    sos = st.segments[-1][1]
    a, n = next((a, n) for m, a, n in st.segments if m in (0xC0, 0xC1))
    seg = bytearray(d[a:a + 2 + n])
    for s, (y, x) in enumerate(((1, 1), (65535, 65535), (struct.unpack_from(">H", seg, 5)[0] + 8, struct.unpack_from(">H", seg, 7)[0] + 16))):
        struct.pack_into(">HH", seg, 5, y, x)           # a second SOF0 of another size, behind the first and in front of the scan
        out.append(_spliced(b, "second-sof", s, a + 2 + n, 0, seg))
        out.append(_spliced(b, "second-sof-first", s, a, 0, seg))
    for s, v in enumerate((0, 1, 2, 8193)):             # a second DRI (the first one where the file has none) in front of the scan
        out.append(_spliced(b, "second-dri", s, sos, 0, b"\xff\xdd\x00\x04" + struct.pack(">H", v)))
    for s, (m, at, n) in enumerate(st.segments):        # a DHT repeated in front of the scan: with another table's contents under
        if m == 0xC4 and at in [a for mm, a, _ in st.segments if mm == 0xC4][:2]:       # its own Tc/Th, and with the values reversed
            others = [(a2, n2) for m2, a2, n2 in st.segments if m2 == 0xC4 and a2 != at and d[a2 + 4] >> 4 == d[at + 4] >> 4]
            for a2, n2 in others[:1]:
                out.append(_spliced(b, "second-dht", 2 * s, sos, 0, d[a2:a2 + 4] + d[at + 4:at + 5] + d[a2 + 5:a2 + 2 + n2]))
            out.append(_spliced(b, "second-dht", 2 * s + 1, sos, 0, d[at:at + 21] + d[at + 21:at + 2 + n][::-1]))
        if m == 0xDB:                                   # and a DQT repeated with every entry 255
            out.append(_spliced(b, "second-dqt", s, sos, 0, d[at:at + 5] + b"\xff" * (n - 3)))
    return out


def scan_mutants(b):
    st, out, d = b.structure(), [], b.data
    rng = np.random.default_rng([b.index, 207])
    scan, end = st.scan, st.end
    nbytes = end - scan
    if nbytes < 1:
        return out
    last = st.intervals()[-1]
    for s in range(SCAN_BITS[b.heavy]):
        pos = scan + int(rng.integers(nbytes))
        out.append(_patched(b, "scan-bit", s, [(pos, bytes([d[pos] ^ 1 << int(rng.integers(8))]))]))
    # FF and a byte that is not 0 over two bytes of the data: RSTn out of order, a foreign marker, EOI early (twice anywhere
    # and twice inside the last interval, where the count of intervals stays what the headers say)
    for s, v in enumerate((0xD0, 0xD5, 0x01, 0xC4, 0xD9, 0xD9)):
        out.append(_patched(b, "scan-marker", s, [(scan + int(rng.integers(max(1, nbytes - 1))), bytes([0xFF, v]))]))
    for s in range(2):
        lo, hi = last
        if hi - lo >= 2:
            out.append(_patched(b, "scan-marker", 6 + s, [(lo + int(rng.integers(max(1, (hi - lo) // 2 if s else hi - lo - 1))), b"\xff\xd9")]))
    out.append(_spliced(b, "scan-marker-inserted", 0, scan + int(rng.integers(nbytes)), 0, bytes([0xFF, 0xD0 + int(rng.integers(8))])))
    out.append(_patched(b, "scan-ff-last", 0, [(end - 1, b"\xff")]))
    for s in range(3):          # sixteen one-bits: FF 00 FF 00 in the stuffed data
        out.append(_patched(b, "scan-ones", s, [(scan + int(rng.integers(max(1, nbytes - 3))), b"\xff\x00\xff\x00")]))
    for s in range(2):
        out.append(_patched(b, "scan-ffff", s, [(scan + int(rng.integers(max(1, nbytes - 1))), b"\xff\xff")]))
    for s, k in enumerate(sorted({1, 2, 1 + int(rng.integers(max(1, (last[1] - last[0]) // 2))), 1 + int(rng.integers(nbytes))})):
        if k <= nbytes:         # the scan less its last k bytes: EOI moves up
            out.append(_spliced(b, "scan-short", s, end - k, k, b""))
    return [m for m in out if m is not None]


@functools.lru_cache(maxsize=None)
def mutants_of(b):
    fields = header_mutants(b)
    if b.name not in FULL_STRUCTURE:
        pick = np.random.default_rng([b.index, 205]).permutation(len(fields))[:STRUCT_SAMPLE]
        fields = [fields[i] for i in sorted(pick)]
    out = blind_mutants(b) + fields + segment_mutants(b) + scan_mutants(b)
    for i, m in enumerate(out):
        m.index = i
    return tuple(out)


# ------------------------------------------------------------------------------------------------ parse, restate, classify
class Outcome:
    """what jpeg.read made of a file: `frames` {split: JpegFrame or None}, `errors` {split: the exception or None}, `where`
    {split: file:line that raised}, `warnings` what the warnings module was given, the three parses' `seconds`, the file's
    length `nbytes`; `mutant` is None for a base"""

    def __init__(self, base, mutant, frames, errors, where, warned, seconds, path, nbytes):
        self.base, self.mutant, self.frames, self.errors, self.where = base, mutant, frames, errors, where
        self.warnings, self.seconds, self.path, self.nbytes = warned, seconds, path, nbytes
        self._key = None

    @property
    def recipe(self):
        return (self.base.name, "base", None, None, None) if self.mutant is None else self.mutant.recipe

    @property
    def data(self):
        return self.base.data if self.mutant is None else self.mutant.data

    @property
    def accepted(self):
        """by jpeg.read(split="always"), which takes every file the other two modes take"""
        return self.frames["always"] is not None

    @property
    def serial(self):
        """accepted at split=None: the file goes to the serial kernel, one lane a restart interval"""
        return self.frames[None] is not None

    @property
    def frame(self):
        return self.frames["always"]

    @property
    def restate(self):
        h, w = self.frame.shape
        return h * w <= MAX_SAMPLES

    def key(self):
        """(headers, scan bytes): what the kernels are given"""
        if self._key is None:
            f = self.frame
            hh = hashlib.blake2b(digest_size=16)
            hh.update(bytes(f.desc))
            hh.update(f.offsets.tobytes())
            hh.update(np.asarray(f.span).tobytes())
            hh.update(b"serial" if self.serial else b"split")
            self._key = hh.digest()
        return self._key


def parse(b, mutant=None):
    """jpeg.read on the file's bytes at every `split`: an Outcome"""
    import warnings
    data = b.data if mutant is None else mutant.data
    path = os.path.join(workdir(), f"{b.index}.jpg")        # (one file per base, written over)
    with open(path, "wb") as fh:
        fh.write(data)
    frames, errors, where = {}, {}, {}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        t0 = time.perf_counter()
        for split in SPLITS:
            frames[split] = errors[split] = where[split] = None
            try:
                frames[split] = jpeg.read(path, split)
            except Exception as exc:        # noqa: BLE001 -- the test decides which exceptions are refusals
                errors[split], tb = exc, exc.__traceback__
                while tb.tb_next is not None:
                    tb = tb.tb_next
                where[split] = f"{os.path.basename(tb.tb_frame.f_code.co_filename)}:{tb.tb_lineno}"
                link = exc                  # (a traceback holds the reader's locals, the mapping among them: let go of every one)
                while link is not None:
                    link.__traceback__, link = None, link.__cause__ or link.__context__
        seconds = time.perf_counter() - t0
    for f in frames.values():
        if f is not None:                   # (a mapping holds a file descriptor, and the file is written over: a copy of the span)
            f.span = np.array(f.span)
            f._keep = None
    return Outcome(b, mutant, frames, errors, where, [str(w.message) for w in caught], seconds, path, len(data))


@functools.lru_cache(maxsize=None)
def base_outcome(b):
    return parse(b)


@functools.lru_cache(maxsize=None)
def outcomes_of(b):
    with _no_collection():
        return tuple(parse(b, m) for m in mutants_of(b))


def outcomes():
    """every mutant of every base, parsed once"""
    return [o for b in bases() for o in outcomes_of(b)]


class Restated:
    """`h` the lenient parser's headers; `serial` (planes, status) of jpeg_restatement.walk, None where split=None refuses the
    file; `split` (planes, status) of jpeg_split_restatement.walk_split; `bgr(which)` render of either, computed on demand"""

    def __init__(self, data, serial):
        self.h = R.parse(data)
        self.serial = self._frozen(R.walk(data, self.h)) if serial else None
        self.split = self._frozen(S.walk_split(data, self.h))
        self._bgr = {}

    @staticmethod
    def _frozen(pair):
        for a in pair[0] + [pair[1]]:
            a.setflags(write=False)
        return pair

    def bgr(self, which):
        if which not in self._bgr:
            self._bgr[which] = R.render(getattr(self, which)[0], self.h)
            self._bgr[which].setflags(write=False)
        return self._bgr[which]

    @property
    def native(self):
        """what the file's own path yields: the serial walk where it has restart intervals, else the split walk"""
        return self.serial if self.serial is not None else self.split


_RESTATED = {}


def restated(outcome):
    """the restatement of an accepted outcome (`Outcome.restate`), once per distinct key, read-only"""
    k = outcome.key()
    if k not in _RESTATED:
        _RESTATED[k] = Restated(outcome.data, outcome.serial)
    return _RESTATED[k]


def changed(outcome):
    """the kernels are given something else than for the base"""
    return outcome.key() != base_outcome(outcome.base).key()


CLASSES = ("differs", "nocode", "overrun", "run", "dht-move", "quant", "marker")


def classes(outcome):
    """Of an accepted, restated mutant, the subset of CLASSES it falls in, by its native walk: "differs" -- status 0 and other
    coefficients (or another geometry) than the base; "nocode", "overrun", "run" -- the status bit, in some interval;
    "dht-move" -- a `dht-move` mutant with status 0 in every interval: a changed table that still decodes; "quant" -- a
    changed quantisation entry that a component selects; "marker" -- a `scan-marker` mutant that is accepted: an EOI in the
    middle of the last interval, whose data then ends early (OVERRUN)"""
    r, rb = restated(outcome), restated(base_outcome(outcome.base))
    (planes, status), (want, _) = r.native, rb.native
    out = set()
    for name, bit in (("nocode", NOCODE), ("overrun", OVERRUN), ("run", RUN)):
        if (status & bit).any():
            out.add(name)
    if not status.any() and (len(planes) != len(want) or any(p.shape != w.shape or not np.array_equal(p, w) for p, w in zip(planes, want))):
        out.add("differs")
    if outcome.mutant.kind == "dht-move" and not status.any() and bytes(outcome.frame.desc) != bytes(base_outcome(outcome.base).frame.desc):
        out.add("dht-move")
    tq = lambda rr: [rr.h["quant"][c[3]][1] for c in rr.h["comps"]]
    if outcome.mutant.kind in ("dqt-entry", "second-dqt") and tq(r) != tq(rb):
        out.add("quant")
    if outcome.mutant.kind == "scan-marker" and (status & OVERRUN).any():
        out.add("marker")
    return out


# ------------------------------------------------------------------------------------------------ what the GPU file runs
CLASS_KINDS = ("dht-move", "dqt-entry", "scan-marker", "scan-bit", "scan-ones", "scan-short", "dht-value", "second-dqt", "second-dht",
               "sof-x", "sof-y", "bit", "byte")
CLASS_TRIES = 12        # candidates restated per base
CELL_PICKS = 2          # mutants per (mode, with or without restart intervals, class)
HEADER_GROUPS = ("sof", "dht", "dqt", "dri", "second-", "sos", "remove-")


def cell(outcome):
    """(the base's sampling, whether the file is read with restart intervals)"""
    return outcome.base.mode, outcome.serial


@functools.lru_cache(maxsize=None)
def class_picks(b):
    """{class: outcome} of a base: the first accepted mutant found in each of CLASSES among at most CLASS_TRIES candidates --
    the accepted, restated mutants of CLASS_KINDS that changed what the kernels are given, the first of every kind, then the
    second of every kind, ...  Only these are restated."""
    rank, cands = {}, []
    for o in outcomes_of(b):
        if o.accepted and o.restate and o.mutant.kind in CLASS_KINDS and changed(o):
            rank[o.mutant.kind] = rank.get(o.mutant.kind, -1) + 1
            cands.append((rank[o.mutant.kind], CLASS_KINDS.index(o.mutant.kind), o))
    found = {}
    for _, _, o in sorted(cands, key=lambda c: c[:2])[:CLASS_TRIES]:
        for c in classes(o):
            found.setdefault(c, o)
    return found


@functools.lru_cache(maxsize=None)
def device_selection():
    """At most DEVICE_LIMIT accepted, restated outcomes, no two with the same (headers, scan bytes): `class_picks` of every
    base until each (mode, with or without restart intervals, class) has CELL_PICKS mutants (a heavy base gives to an empty
    cell only), then of every base that is not heavy one accepted mutant that changed a header the kernels take (size,
    selectors, DRI, tables, quantisation; HEADER_GROUPS in turn), and for what is left of the limit a seeded sample of every other
    accepted mutant of those bases that changed what the kernels are given."""
    picked, seen, have = [], set(), {}

    def take(o):
        if len(picked) < DEVICE_LIMIT and o.key() not in seen:
            seen.add(o.key())
            picked.append(o)
            return True
        return False

    for b in sorted(bases(), key=lambda b: b.heavy):
        for c, o in class_picks(b).items():
            k = cell(o) + (c,)
            if have.get(k, 0) < (1 if b.heavy else CELL_PICKS) and take(o):
                have[k] = have.get(k, 0) + 1
    rest = []
    for b in bases():
        if b.heavy:
            continue
        mine = [o for o in outcomes_of(b) if o.accepted and o.restate and changed(o)]
        own = bytes(base_outcome(b).frame.desc)
        heads = [o for o in mine if bytes(o.frame.desc) != own and not o.mutant.blind]
        group = HEADER_GROUPS[b.index % len(HEADER_GROUPS)]     # (which segment's mutant is asked of a base goes round)
        for o in [o for o in heads if o.mutant.kind.startswith(group)][:1] or heads[:1]:
            take(o)
        rest += mine
    for i in np.random.default_rng(209).permutation(len(rest)):
        take(rest[i])
    return tuple(picked)
