"""The baseline-JPEG decoder restated in NumPy, integers only: the definition the kernels (csrc/kernels_jpeg.hpp,
csrc/jpeg_core.hpp) are held to, bit for bit, and the thing that is pinned against libjpeg-turbo (tests/test_jpeg_host.py).
Serial where the stream is serial, bits as one Python int; no cleverness.

    parse       the marker segments by their lengths, first frame only; lenient: it reads whatever has the shape of a
                baseline file and leaves refusing to shinestacker_amd.jpeg.read
    intervals   the scan is searched for FF followed by anything but 00: each D0 .. D7 starts the next interval behind it, the
                first other marker ends the scan; offsets[i] is interval i's first byte, offsets[n] the scan's end
    bits        most significant bit first; FF 00 is the byte FF; FF before anything else ends the interval (an FF that is the
                interval's very last byte reads as FF); every bit beyond the end counts as 0
    block       DC: category s from the component's DC table (a symbol above 15 counts as no code), the s bits behind it
                extended (T.81 F.2.2.1), the coefficient the running sum mod 2^16 as int16.  AC from k = 1: rs = (r << 4) | s;
                s == 0 and r == 15: k += 16 (k past 63: status bit 2); s == 0 otherwise: end of block; else k += r, the s
                bits are taken, k <= 63: coef[zigzag[k]] = extend(bits, s), k > 63: dropped with status bit 2; k += 1.  The
                block ends once k passes 63.
    status      per interval: bit 0 a 16-bit prefix matched no code (symbol 0 behind 16 bits), bit 1 bits were taken from
                beyond the interval's end, bit 2 a run carried k past 63
    order       interval i holds min(DRI, MCUs left) MCUs from MCU i * DRI on, in scan order; blocks of an MCU in T.81 order
                (component by component, rows of its v x h blocks); predictors 0 at the interval's start
    idct        coefficient times table entry, then the 13-bit slow-integer form: columns descaled by 11, rows by 18, both
                with rounding, + 128, clipped to 0 .. 255; int64 throughout
    upsample    on the component cropped to ceil(H v / vmax) x ceil(W h / hmax); a component of 1 or 2 samples a row is
                replicated, 2 x 1 or 2 x 2, as libjpeg does it; a wider one is filtered, edges replicated: 2:1 horizontal
                (3a + left + 1) >> 2 and (3a + right + 2) >> 2; 2:1 both ways t = 3 near_row + far_row, then
                (3t + t_left + 8) >> 4 and (3t + t_right + 7) >> 4
    colour      R = Y + ((91881 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16),
                G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16), primes minus 128, shifts arithmetic, clipped, stored BGR;
                grey: the plane three times
"""
import struct

import numpy as np

NOCODE, OVERRUN, RUN = 1, 2, 4
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def codes(counts, values):
    """{(length, code): symbol}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[(length, code)] = values[k]
            code += 1
            k += 1
        code <<= 1
    return out


def unstuff(data):
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


def intervals(data, scan_off):
    """(offsets: interval starts and the scan's end, the markers met in order)"""
    offs, marks, i = [scan_off], [], scan_off
    while i + 1 < len(data):
        if data[i] == 0xFF and data[i + 1] != 0:
            m = data[i + 1]
            if 0xD0 <= m <= 0xD7:
                marks.append(m)
                offs.append(i + 2)
                i += 2
                continue
            return offs + [i], marks
        i += 1
    return offs + [len(data)], marks


def parse(data):
    """the headers of a baseline file: a dict; ValueError where nothing can be read"""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    h = {"quant": {}, "tables": {}, "dri": 0, "jfif": False, "adobe": None, "orientation": 1, "sof": None}
    pos = 2
    while pos + 4 <= len(data):
        if data[pos] != 0xFF:
            raise ValueError(f"no marker at {pos}")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        body = data[pos + 4:pos + 2 + n]
        if m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq:
                    vals = struct.unpack(">64H", body[q + 1:q + 129])
                    q += 129
                else:
                    vals = body[q + 1:q + 65]
                    q += 65
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = vals[k]
                h["quant"][tq] = (pq, nat)
        elif m == 0xC4:
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                counts = list(body[q + 1:q + 17])
                values = list(body[q + 17:q + 17 + sum(counts)])
                q += 17 + sum(counts)
                h["tables"][(tc, th)] = (counts, values)
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if h["sof"] is None:
                p, y, x, nf = struct.unpack(">BHHB", body[:6])
                h.update(sof=m, precision=p, height=y, width=x,
                         comps=[(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nf)])
        elif m == 0xDD:
            h["dri"] = struct.unpack(">H", body[:2])[0]
        elif m == 0xE0 and body[:5] == b"JFIF\0":
            h["jfif"] = True
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            h["adobe"] = body[11]
        elif m == 0xE1 and body[:6] == b"Exif\0\0":
            h["orientation"] = _orientation(body[6:])
        elif m == 0xDA:
            ns = body[0]
            h["scan"] = [(body[1 + 2 * c], body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(ns)]
            h["scan_off"] = pos + 2 + n
            break
        pos += 2 + n
    if h["sof"] is None or "scan" not in h:
        raise ValueError("no frame or no scan")
    h["offsets"], h["markers"] = intervals(data, h["scan_off"])
    nf = len(h["comps"])
    h["ncomp"] = nf
    h["hmax"], h["vmax"] = (h["comps"][0][1], h["comps"][0][2]) if nf > 1 else (1, 1)
    return h


def _orientation(tiff):
    try:
        e = "<" if tiff[:2] == b"II" else ">"
        off = struct.unpack(e + "I", tiff[4:8])[0]
        for i in range(struct.unpack(e + "H", tiff[off:off + 2])[0]):
            tag, typ, cnt = struct.unpack(e + "HHI", tiff[off + 2 + 12 * i:off + 10 + 12 * i])
            if tag == 0x0112 and typ == 3:
                return struct.unpack(e + "H", tiff[off + 10 + 12 * i:off + 12 + 12 * i])[0]
    except struct.error:
        pass
    return 1


def geometry(h):
    """per component (h, v, blocks wide, blocks high, own width, own height), and the MCU grid"""
    W, H, hm, vm = h["width"], h["height"], h["hmax"], h["vmax"]
    mx, my = -(-W // (8 * hm)), -(-H // (8 * vm))
    comps = []
    for c in range(h["ncomp"]):
        ch, cv = (hm, vm) if c == 0 else (1, 1)
        comps.append((ch, cv, mx * ch, my * cv, -(-W * ch // hm), -(-H * cv // vm)))
    return comps, mx, my


def extend(v, s):
    return v if v >= 1 << (s - 1) else (v - ((1 << s) - 1)) & 0xFFFF


def _s16(v):
    return v - 65536 if v >= 32768 else v


def walk(data, h, dri=None, trace=None):
    """(per component its (bh, bw, 64) int16 coefficient plane, the uint32 status words).  `trace`: a set that collects what
    the streams really contained ("zrl", "len16", "cat15", "noeob", "ff-first", ...)"""
    data = bytes(data)
    comps, mx, my = geometry(h)
    dri = h["dri"] if dri is None else dri
    n_mcus = mx * my
    offs = h["offsets"]
    n_int = len(offs) - 1
    planes = [np.zeros((bh, bw, 64), np.int16) for (_, _, bw, bh, _, _) in comps]
    status = np.zeros(n_int, np.uint32)
    sel = []
    for c in range(h["ncomp"]):
        _, td, ta = h["scan"][c]
        sel.append((codes(*h["tables"].get((0, td), ([0] * 16, []))), codes(*h["tables"].get((1, ta), ([0] * 16, [])))))
    trace = set() if trace is None else trace
    for i in range(n_int):
        raw = data[offs[i]:offs[i + 1]]
        real = unstuff(raw)
        if trace is not None and len(real):
            for name, at in (("ff-first", 0), ("ff-last", len(real) - 1)):
                if real[at] == 0xFF:
                    trace.add(name)
            if 0xFF in real[1:-1]:
                trace.add("ff-middle")
        nbits = 8 * len(real)
        big = int.from_bytes(real, "big") if real else 0
        pos = 0
        st = 0

        def bits(at, n):
            end = at + n
            if end <= nbits:
                return (big >> (nbits - end)) & ((1 << n) - 1)
            if at >= nbits:
                return 0
            return ((big & ((1 << (nbits - at)) - 1)) << (end - nbits)) & ((1 << n) - 1)

        def symbol(tab):
            nonlocal pos, st
            peek = bits(pos, 16)
            for length in range(1, 17):
                key = (length, peek >> (16 - length))
                if key in tab:
                    pos += length
                    if length == 16:
                        trace.add("len16")
                    return tab[key]
            st |= NOCODE
            pos += 16
            return None
        pred = [0] * h["ncomp"]
        for mcu in range(i * dri, min((i + 1) * dri, n_mcus)):
            row, col = divmod(mcu, mx)
            for c, (ch, cv, bw, bh, _, _) in enumerate(comps):
                dc, ac = sel[c]
                for by in range(cv):
                    for bx in range(ch):
                        blk = planes[c][row * cv + by, col * ch + bx]
                        blk[:] = 0
                        s = symbol(dc)
                        if s is None:
                            s = 0
                        elif s > 15:
                            st |= NOCODE
                            s = 0
                        if s:
                            if s == 15:
                                trace.add("dc-cat15")
                            pred[c] = (pred[c] + extend(bits(pos, s), s)) & 0xFFFF
                            pos += s
                        blk[0] = _s16(pred[c])
                        k = 1
                        eob = False
                        for _ in range(63):
                            rs = symbol(ac)
                            rs = 0 if rs is None else rs
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r == 15:
                                    trace.add("zrl")
                                    k += 16
                                    if k > 63:
                                        st |= RUN
                                else:
                                    eob = True
                                    break
                            else:
                                if s == 15:
                                    trace.add("cat15")
                                k += r
                                v = extend(bits(pos, s), s)
                                pos += s
                                if k <= 63:
                                    blk[ZIGZAG[k]] = _s16(v)
                                else:
                                    st |= RUN
                                k += 1
                            if k > 63:
                                break
                        if not eob and not st:
                            trace.add("noeob")
        if pos > nbits:
            st |= OVERRUN
        status[i] = st
    return planes, status


C = (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172)


def _idct8(x):
    """one pass over axis 0 of an (8, ...) int64 array, before the descale"""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[0] + x[4]) * 8192
    tmp1 = (x[0] - x[4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3])


def idct(coef, quant):
    """(..., 64) int16 coefficients and 64 table entries, both in natural order -> (..., 8, 8) uint8 samples"""
    x = coef.astype(np.int64) * np.asarray(quant, np.int64)
    x = x.reshape(x.shape[:-1] + (8, 8))
    cols = (_idct8(np.moveaxis(x, -2, 0)) + (1 << 10)) >> 11            # (v, ..., u): the column pass
    rows = (_idct8(np.moveaxis(cols, -1, 0)) + (1 << 17)) >> 18         # (x, v, ...)
    out = np.clip(rows + 128, 0, 255).astype(np.uint8)
    return np.moveaxis(np.moveaxis(out, 0, -1), 0, -2)                  # (..., v, x)


def plane(coef_plane, quant):
    """a component's (bh, bw, 64) coefficients -> its padded (bh * 8, bw * 8) sample plane"""
    s = idct(coef_plane, quant)
    bh, bw = s.shape[:2]
    return s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample(p, hm, vm, H, W):
    """a chroma component cropped to its own size -> H x W int64"""
    p = p.astype(np.int64)
    if hm == 1:
        return p[:H, :W]
    if p.shape[1] <= 2:         # libjpeg filters only a component more than 2 samples wide: plain replication, both ways
        return np.repeat(np.repeat(p, vm, axis=0), 2, axis=1)[:H, :W]
    if vm == 2:
        near = np.repeat(p, 2, axis=0)
        up, down = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
        far = np.empty_like(near)
        far[0::2], far[1::2] = up, down
        t, a, b = 3 * near + far, 8, 7
    else:
        t, a, b = p, 1, 2
    left, right = np.hstack([t[:, :1], t[:, :-1]]), np.hstack([t[:, 1:], t[:, -1:]])
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int64)
    sh = 4 if vm == 2 else 2
    out[:, 0::2] = (3 * t + left + a) >> sh
    out[:, 1::2] = (3 * t + right + b) >> sh
    return out[:H, :W]


def colour(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def render(planes, h):
    """coefficient planes -> H x W x 3 BGR uint8"""
    comps, _, _ = geometry(h)
    W, H = h["width"], h["height"]
    samples = [plane(planes[c], h["quant"][h["comps"][c][3]][1]) for c in range(h["ncomp"])]
    y = samples[0][:H, :W]
    if h["ncomp"] == 1:
        return np.repeat(y[:, :, None], 3, 2)
    chroma = [upsample(samples[c][:comps[c][5], :comps[c][4]], h["hmax"], h["vmax"], H, W) for c in (1, 2)]
    return colour(y, *chroma)


def decode(data, trace=None):
    """(H x W x 3 BGR uint8, status words) of a file's bytes"""
    h = parse(data)
    planes, status = walk(data, h, trace=trace)
    return render(planes, h), status
