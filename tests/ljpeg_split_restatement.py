"""The split lossless-JPEG decoder (csrc/ljpeg_sync_core.hpp, csrc/kernels_ljpeg_split.hpp) restated in Python: a segment of
any length is cut into subsequences, every one is decoded from a guess, and the guesses are repaired until each lane's entry
is its predecessor's exit; the differences that come out become samples by prediction afterwards.  Serial, with a byte-wise
bit reader (five unstuffed bytes a symbol), so that it stays linear in the stream's length.  The definition the kernels and
tools/ljpeg_split_check.cpp are held to, bit for bit; tests/test_ljpeg_split_host.py holds it to tests/ljpeg_restatement.py.

    data         a segment's bytes span[scan_off : scan_off + scan_bytes], cut at the span's end.  They end at the first FF
                 followed by anything but 00 (an FF that is the very last byte reads as FF); bits beyond the end are 0.
    state        (p, q, c) at a symbol boundary: p the byte of the data that holds the next unread bit (never the 00 of an FF 00
                 pair), q the bits of it already read, c the component of the next sample; or END once a symbol would start
                 at or beyond the data's end.
    symbol       the category s whose code in component c's table leads the next 16 bits -- none, or s > 16, counts as
                 category 0 behind 16 bits (no code: 16 bits; s > 16: the code's length) with NOCODE --, s = 16: 32768, else s
                 bits v: v when v >= 2^(s-1), v - (2^s - 1) otherwise, mod 2^16.  A symbol that takes bits from beyond the
                 end sets OVERRUN and leaves the state at the end, so that the next one is END.
    subsequence  j of a segment holds its bytes j * sub_bytes .. (j + 1) * sub_bytes (the last one is shorter; a segment of no
                 bytes has one subsequence of none) and owns the symbols whose first bit lies in it; the last one owns
                 everything behind it as well.  Its cold state is (its first byte -- one later where that is a stuffed 00 --,
                 0, 0).  A lane whose entry lies beyond its subsequence decodes nothing and passes the state through.
    differences  the serial walk with the true states: the segment has a quota of rows * columns samples; symbols behind the
                 quota count for nothing; the walk ends at END, with OVERRUN when the quota was not reached.  Unreached
                 differences are 0.
    rounds       round 0: every workgroup of `group` consecutive subsequences (of all segments, segment after segment)
                 converges on its own, its first lane cold unless it is a segment's first.  Round r: every workgroup converges
                 again from the exit its predecessor had after round r - 1.  rounds_needed is the number of rounds behind
                 round 0 after which every exit is the true one.
    prediction   ljpeg_restatement's, on the plane of differences: predictor 1 is a sum down the first ncomp columns from
                 2^(P-1) and then a sum along every row per component, mod 2^16.
"""
import numpy as np

import ljpeg_restatement as R

NOCODE, OVERRUN, UNDECODED, UNSYNCED = 1, 2, 4, 8
END = None
GROUP = 256


class Data:
    """a segment's bytes, prepared: `real` the unstuffed data bytes, `raw_of[u]` the byte that holds unstuffed byte u
    (raw_of[len(real)] is the data's end), `u_of` the inverse for the bytes that start one"""

    def __init__(self, raw):
        self.raw = raw = bytes(raw)
        real, raw_of, i = bytearray(), [], 0
        while i < len(raw):
            b = raw[i]
            nxt = raw[i + 1] if i + 1 < len(raw) else 0
            if b == 0xFF and nxt != 0:
                break
            real.append(b)
            raw_of.append(i)
            i += 2 if (b == 0xFF and i + 1 < len(raw)) else 1
        self.end = i
        self.real = bytes(real) + bytes(8)
        self.nreal = len(real)
        self.raw_of = raw_of + [i]
        self.u_of = {p: u for u, p in enumerate(self.raw_of)}


class Segment:
    """one segment: its Data, the components' tables ({(length, code): category}), ncomp, predictor, precision, rows, columns"""

    def __init__(self, raw, tables, ncomp, predictor, precision, rows, cols):
        self.data = Data(raw)
        self.tabs = [_by_prefix(R.codes(c, v)) for c, v in tables]
        self.ncomp, self.predictor, self.precision, self.rows, self.cols = ncomp, predictor, precision, rows, cols

    @property
    def quota(self):
        return self.rows * self.cols


def _by_prefix(tab):
    """the codes of a table as a list, shortest first: [(length, code, category)]"""
    return sorted((length, code, s) for (length, code), s in tab.items())


def _lookup(tab, peek):
    for length, code, s in tab:
        if peek >> (16 - length) == code:
            return s, length
    return None, 16


def symbol(seg, state):
    """one symbol from `state` (not END): (the next state, (status bits, the difference mod 2^16)); (END, None) when it would
    start at or beyond the data's end"""
    d = seg.data
    p, q, c = state
    u = d.u_of.get(p)
    if u is None or u >= d.nreal:
        return END, None
    w = int.from_bytes(d.real[u:u + 5], "big")
    peek = (w >> (24 - q)) & 0xFFFF
    s, length = _lookup(seg.tabs[c], peek)
    st = 0
    if s is None or s > 16:
        st, s = NOCODE, 0
    extra = s if s < 16 else 0
    val = 32768 if s == 16 else 0
    if extra:
        v = (w >> (40 - q - length - extra)) & ((1 << extra) - 1)
        val = (v if v >= 1 << (extra - 1) else v - ((1 << extra) - 1)) & 0xFFFF
    t = q + length + extra
    if t > 8 * (d.nreal - u):
        st |= OVERRUN
        p, q = d.end, 0
    else:
        p, q = d.raw_of[u + (t >> 3)], t & 7
    return (p, q, (c + 1) % seg.ncomp), (st, val)


def subsequences(length, sub_bytes):
    """[(first byte, byte behind the last)] of a segment of `length` bytes: at least one"""
    n = max(1, -(-length // sub_bytes))
    return [(j * sub_bytes, min((j + 1) * sub_bytes, length)) for j in range(n)]


def cold(seg, lo):
    raw = seg.data.raw
    return (lo + 1 if 0 < lo < len(raw) and raw[lo - 1] == 0xFF and raw[lo] == 0 else lo, 0, 0)


def lane(seg, hi, last, entry, emit=None):
    """subsequence .. hi from `entry`: (exit state, samples decoded).  `emit(what the symbol did, or None at END)`"""
    st, n = entry, 0
    while st is not END and (last or st[0] < hi):
        nxt, did = symbol(seg, st)
        if nxt is END:
            if emit is not None:
                emit(None)
            st = END
            break
        if emit is not None:
            emit(did)
        n += 1
        st = nxt
    return st, n


def differences(seg):
    """(the rows x columns uint16 plane of differences, the status word) of one segment, walked with the true states"""
    quota = seg.quota
    out = np.zeros(quota, np.uint16)
    box = [0, 0]

    def emit(did):
        if box[0] >= quota:
            return
        if did is None:
            box[1] |= OVERRUN
            return
        box[1] |= did[0]
        out[box[0]] = did[1]
        box[0] += 1
    lane(seg, len(seg.data.raw), True, (0, 0, 0), emit)
    return out.reshape(seg.rows, seg.cols), box[1]


def predict(diff, ncomp, predictor, precision):
    """the samples (int64, mod 2^16) of a plane of differences"""
    d = np.asarray(diff, np.int64)
    rows, w = d.shape
    if predictor == 1:
        v = d.copy()
        v[0, :ncomp] += 1 << (precision - 1)
        v[:, :ncomp] = np.cumsum(v[:, :ncomp], axis=0) & 0xFFFF        # down the first columns from the seed
        for c in range(ncomp):
            v[:, c::ncomp] = np.cumsum(v[:, c::ncomp], axis=1) & 0xFFFF
        return v
    out = np.zeros((rows, w), np.int64)
    for r in range(rows):
        for col in range(w):
            if r == 0 and col < ncomp:
                px = 1 << (precision - 1)
            elif r == 0:
                px = int(out[0, col - ncomp])
            elif col < ncomp:
                px = int(out[r - 1, col])
            else:
                ra, rb, rc = int(out[r, col - ncomp]), int(out[r - 1, col]), int(out[r - 1, col - ncomp])
                px = {2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1), 7: (ra + rb) >> 1}[predictor]
            out[r, col] = (px + int(d[r, col])) & 0xFFFF
    return out


def decode(seg):
    """(samples, status) of one segment: ljpeg_restatement.decode's result by the split decoder's route"""
    diff, status = differences(seg)
    return predict(diff, seg.ncomp, seg.predictor, seg.precision), status


def segments_of(span, layout):
    """the Segments of a shinestacker_amd.dng.RawLayout (only its fields are read) over `span`, in grid order"""
    span = bytes(np.asarray(span, np.uint8))
    out = []
    for k, s in enumerate(layout.segments):
        nc = int(s["ncomp"])
        tables = [([int(v) for v in s["counts"][c]], [int(v) for v in s["values"][c]]) for c in range(nc)]
        raw = span[int(s["scan_off"]):int(s["scan_off"]) + int(s["scan_bytes"])]
        out.append(Segment(raw, tables, nc, int(s["predictor"]), int(s["precision"]), layout.segment_rows(k), layout.seg_width))
    return out


def unpack_layout(span, layout):
    """(the cropped mosaic, the status words, per segment its plane of differences): ljpeg_restatement.unpack_layout's
    result by the split decoder's route"""
    nsx = -(-layout.image_width // layout.seg_width)
    dtype = np.dtype(layout.dtype)
    maxv = int(np.iinfo(dtype).max)
    out = np.zeros((layout.height, layout.width), dtype)
    segs = segments_of(span, layout)
    status = np.zeros(len(segs), np.uint32)
    planes = []
    for k, seg in enumerate(segs):
        diff, status[k] = differences(seg)
        planes.append(diff)
        v = predict(diff, seg.ncomp, seg.predictor, seg.precision)
        if layout.table is not None:
            v = np.asarray(layout.table, np.int64)[np.minimum(v, len(layout.table) - 1)]
        v = ((v << layout.shift) & maxv).astype(dtype)
        y0, x0 = (k // nsx) * layout.seg_height - layout.crop_y, (k % nsx) * layout.seg_width - layout.crop_x
        ys, xs = np.arange(seg.rows) + y0, np.arange(seg.cols) + x0
        ky, kx = (ys >= 0) & (ys < layout.height), (xs >= 0) & (xs < layout.width)
        out[np.ix_(ys[ky], xs[kx])] = v[np.ix_(ky, kx)]
    return out, status, planes


def lanes_of(segs, sub_bytes):
    """every subsequence of the segments in order: (Segment, first byte, byte behind the last, is the segment's last)"""
    out = []
    for seg in segs:
        subs = subsequences(len(seg.data.raw), sub_bytes)
        out += [(seg, lo, hi, j == len(subs) - 1) for j, (lo, hi) in enumerate(subs)]
    return out


def exits(segs, sub_bytes):
    """per subsequence (the exit state and sample count from its cold state, ... from its true entry)"""
    out, prev = [], None
    for seg, lo, hi, last in lanes_of(segs, sub_bytes):
        true_in = (0, 0, 0) if lo == 0 else prev
        true_out = lane(seg, hi, last, true_in)
        out.append((lane(seg, hi, last, cold(seg, lo)), true_out))
        prev = true_out[0]
    return out


def groups_touched(segs, sub_bytes, group=GROUP):
    """the largest number of workgroups any one segment's lanes lie in: that many rounds, less one, always suffice"""
    at, most = 0, 1
    for seg in segs:
        n = len(subsequences(len(seg.data.raw), sub_bytes))
        most = max(most, (at + n - 1) // group - at // group + 1)
        at += n
    return most


def rounds_needed(segs, sub_bytes, group=GROUP):
    """the rounds behind round 0 until every exit is the true one (the module docstring)"""
    L = lanes_of(segs, sub_bytes)
    n = len(L)
    memo = {}

    def f(g, entry):
        key = (g, entry)
        if key not in memo:
            seg, lo, hi, last = L[g]
            memo[key] = lane(seg, hi, last, entry)[0]
        return memo[key]
    ex = [None] * n
    starts = list(range(0, n, group))

    def converge(g0, entry):
        e = entry
        for g in range(g0, min(g0 + group, n)):
            e = f(g, (0, 0, 0) if L[g][1] == 0 else e)
            ex[g] = e
    for g0 in starts:
        converge(g0, cold(L[g0][0], L[g0][1]))
    true = []
    e = None
    for g in range(n):
        e = f(g, (0, 0, 0) if L[g][1] == 0 else e)
        true.append(e)
    rounds = 0
    while ex != true:
        rounds += 1
        assert rounds <= len(starts), "the fix point must be reached after groups - 1 rounds"
        before = list(ex)
        for g0 in starts[1:]:
            converge(g0, before[g0 - 1])
    return rounds


def pass_through_lanes(segs, sub_bytes):
    """the lanes whose true entry is END or lies at or beyond their subsequence's end: they decode nothing.  (A symbol takes at
    most 38 bits from its first byte on, four whole bytes and eight source bytes when all are stuffed, so from sub_bytes 8
    upwards a true entry never jumps a whole subsequence: the lanes that pass a state through are those behind the data's end.)"""
    n, prev = 0, None
    for seg, lo, hi, last in lanes_of(segs, sub_bytes):
        entry = (0, 0, 0) if lo == 0 else prev
        if entry is END or (not last and entry[0] >= hi):
            n += 1
        prev = lane(seg, hi, last, entry)[0]
    return n
