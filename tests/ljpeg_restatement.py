"""raw_ljpeg restated in Python: the definition the kernel (csrc/kernels_ljpeg.hpp, csrc/ljpeg_core.hpp) is held to, bit for
bit.  Serial, one sample at a time, bits as one Python int; no cleverness.

    stream      every strip or tile is one JPEG stream: SOI, DHT segments, SOF3, SOS, entropy-coded data, EOI.  `parse` takes
                precision P, lines Y, samples per line X, components Nf, each component's table (16 counts, the values in code
                order), the predictor Ss and the point transform Al from the headers, and where the data starts.
    bits        the data bytes most significant bit first; FF 00 yields the byte FF; FF before anything else is a marker and
                ends the data; every bit at or beyond the marker, the data's length or the span's end counts as 0
    codes       canonical (T.81 Annex C): code = 0; for each length 1 .. 16: the length's values take consecutive codes in
                order, then code <<= 1
    sample      the category s whose code leads the next bits; s = 0: difference 0; s = 16: 32768 and no further bits;
                otherwise the next s bits v: the difference is v when v >= 2^(s-1) and v - (2^s - 1) otherwise
    order       lines top to bottom, x = 0 .. X-1 within a line, components c = 0 .. Nf-1 within x; the sample lands at
                segment row r, column x * Nf + c
    prediction  per component, Ra the sample Nf columns to the left, Rb above, Rc above-left: 2^(P-1) for the first sample, Ra
                on the rest of the first line, Rb for the first sample of every other line, elsewhere the predictor: 1 Ra,
                2 Rb, 3 Rc, 4 Ra + Rb - Rc, 5 Ra + ((Rb - Rc) >> 1), 6 Rb + ((Ra - Rc) >> 1), 7 (Ra + Rb) >> 1, the shift
                arithmetic.  value = (prediction + difference) mod 2^16
    then        as raw_unpack: v = table[min(v, len - 1)] with a table; out = (v << shift) truncated to the dtype; written at
                (ys - crop_y, xs - crop_x) when the stored site lies inside the crop
    status      per segment: bit 0 a 16-bit prefix matched no code (the sample then counts as category 0 behind 16 bits: what
                follows is unspecified, and bounded); bit 1 the last sample needed bits from beyond the end of the data
"""
import numpy as np

NOCODE, OVERRUN = 1, 2
SOF_NAMES = {0xC0: "SOF0 baseline DCT", 0xC1: "SOF1 extended sequential DCT", 0xC2: "SOF2 progressive DCT", 0xC5: "SOF5 differential DCT",
             0xC6: "SOF6 differential progressive DCT", 0xC7: "SOF7 differential lossless", 0xC9: "SOF9 arithmetic DCT",
             0xCA: "SOF10 arithmetic progressive DCT", 0xCB: "SOF11 arithmetic lossless", 0xCD: "SOF13 differential arithmetic DCT",
             0xCE: "SOF14 differential arithmetic progressive DCT", 0xCF: "SOF15 differential arithmetic lossless"}


def codes(counts, values):
    """{(length, code): category}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[(length, code)] = values[k]
            code += 1
            k += 1
        code <<= 1
    return out


def unstuff(data):
    """the bytes in front of the first marker with FF 00 read as FF (an FF that is the data's very last byte has nothing but
    zeros behind it and reads as FF too)"""
    out, i = bytearray(), 0
    while i < len(data):
        b = data[i]
        if b == 0xFF:
            if (data[i + 1] if i + 1 < len(data) else 0) != 0:
                break
            i += 1
        out.append(b)
        i += 1
    return bytes(out)


def decode(data, tables, precision, lines, x, ncomp, predictor):
    """(lines x (x * ncomp) int64 samples, status) of one segment.  data: the entropy-coded bytes (whatever follows a marker
    is not looked at); tables: per component (counts, values)."""
    real = unstuff(bytes(data))
    nbits = 8 * len(real)
    big = int.from_bytes(real, "big") if real else 0
    pos = 0

    def bits(at, n):        # n bits from bit `at`, zeros beyond the end
        end = at + n
        if end <= nbits:
            return (big >> (nbits - end)) & ((1 << n) - 1)
        if at >= nbits:
            return 0
        return ((big & ((1 << (nbits - at)) - 1)) << (end - nbits)) & ((1 << n) - 1)
    tabs = [codes(c, v) for c, v in tables]
    w = x * ncomp
    out = np.zeros((lines, w), np.int64)
    status = 0
    for r in range(lines):
        for col in range(w):
            tab = tabs[col % ncomp]
            peek = bits(pos, 16)
            s = None
            for length in range(1, 17):
                if (length, peek >> (16 - length)) in tab:
                    s = tab[(length, peek >> (16 - length))]
                    pos += length
                    break
            if s is None or s > 16:
                status |= NOCODE
                pos += 16 if s is None else 0
                s = 0
            if s == 0:
                diff = 0
            elif s == 16:
                diff = 32768
            else:
                v = bits(pos, s)
                pos += s
                diff = v if v >= 1 << (s - 1) else v - ((1 << s) - 1)
            if r == 0 and col < ncomp:
                px = 1 << (precision - 1)
            elif r == 0:
                px = int(out[0, col - ncomp])
            elif col < ncomp:
                px = int(out[r - 1, col])
            else:
                ra, rb, rc = int(out[r, col - ncomp]), int(out[r - 1, col]), int(out[r - 1, col - ncomp])
                px = {1: ra, 2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1), 7: (ra + rb) >> 1}[predictor]
            out[r, col] = (px + diff) & 0xFFFF
    if pos > nbits:
        status |= OVERRUN
    return out, status


def parse(stream):
    """the headers of one JPEG stream (bytes): {"precision", "lines", "x", "ncomp", "tables": per component (counts, values),
    "predictor", "al", "scan_off": where the entropy-coded data starts}.  Raises ValueError on what the decoder does not take."""
    if stream[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    at, dht, frame, dri = 2, {}, None, 0
    while True:
        if at + 4 > len(stream) or stream[at] != 0xFF:
            raise ValueError(f"no marker at {at}")
        m = stream[at + 1]
        if m == 0xFF:       # a fill byte
            at += 1
            continue
        n = stream[at + 2] << 8 | stream[at + 3]
        body = stream[at + 4:at + 2 + n]
        if m == 0xC4:
            i = 0
            while i < len(body):
                th = body[i] & 15
                counts = list(body[i + 1:i + 17])
                values = list(body[i + 17:i + 17 + sum(counts)])
                dht[th] = (counts, values)
                i += 17 + sum(counts)
        elif m == 0xC3:
            frame = {"precision": body[0], "lines": body[1] << 8 | body[2], "x": body[3] << 8 | body[4], "ncomp": body[5],
                     "ids": [body[6 + 3 * i] for i in range(body[5])]}
        elif m in SOF_NAMES:
            raise ValueError(SOF_NAMES[m])
        elif m == 0xDD:
            dri = body[0] << 8 | body[1]
        elif m == 0xDA:
            ns = body[0]
            sel = {body[1 + 2 * i]: body[2 + 2 * i] >> 4 for i in range(ns)}
            if frame is None or ns != frame["ncomp"] or dri:
                raise ValueError("scan without its frame, or a restart interval")
            return {"precision": frame["precision"], "lines": frame["lines"], "x": frame["x"], "ncomp": ns,
                    "tables": [dht[sel[c]] for c in frame["ids"]], "predictor": body[1 + 2 * ns], "al": body[3 + 2 * ns] & 15,
                    "scan_off": at + 2 + n}
        at += 2 + n


def decode_stream(stream):
    """(samples, status) of one whole JPEG stream"""
    p = parse(stream)
    return decode(stream[p["scan_off"]:], p["tables"], p["precision"], p["lines"], p["x"], p["ncomp"], p["predictor"])


def unpack(span, segs, image_h, image_w, seg_h, seg_w, crop_y, crop_x, h, w, shift, table, dtype):
    """(the cropped h x w mosaic, the status of every segment).  segs: one record per segment in grid order with scan_off,
    scan_bytes, x, y, ncomp, predictor, precision, counts[2][16], values[2][17] (mi_ljpeg_seg_t); the data of a segment is
    span[scan_off : scan_off + scan_bytes], cut at the span's end."""
    span = bytes(np.asarray(span, np.uint8))
    nsx, nsy = -(-image_w // seg_w), -(-image_h // seg_h)
    dtype = np.dtype(dtype)
    maxv = int(np.iinfo(dtype).max)
    out = np.zeros((h, w), dtype)
    status = np.zeros(nsx * nsy, np.uint32)
    for k in range(nsx * nsy):
        s = segs[k]
        nc = int(s["ncomp"])
        tables = [([int(v) for v in s["counts"][c]], [int(v) for v in s["values"][c]]) for c in range(nc)]
        data = span[int(s["scan_off"]):int(s["scan_off"]) + int(s["scan_bytes"])]
        vals, status[k] = decode(data, tables, int(s["precision"]), int(s["y"]), int(s["x"]), nc, int(s["predictor"]))
        y0, x0 = (k // nsx) * seg_h, (k % nsx) * seg_w
        for r in range(vals.shape[0]):
            for col in range(vals.shape[1]):
                y, x = y0 + r - crop_y, x0 + col - crop_x
                if 0 <= y < h and 0 <= x < w:
                    v = int(vals[r, col])
                    if table is not None:
                        v = int(table[min(v, len(table) - 1)])
                    out[y, x] = (v << shift) & maxv
    return out, status


def unpack_layout(span, layout):
    """`unpack` for a shinestacker_amd.dng.RawLayout (only its fields are read)"""
    return unpack(span, layout.segments, layout.image_height, layout.image_width, layout.seg_height, layout.seg_width, layout.crop_y,
                  layout.crop_x, layout.height, layout.width, layout.shift, layout.table, layout.dtype)
