"""An independent baseline-JPEG writer and the case table of the device JPEG decoder's tests.

The writer shares nothing with the decoder or its restatement: forward DCT in float64, quantisation, Huffman coding with
GIVEN tables (built here: two DC tables of all 16 categories and two AC tables of all 256 symbols, one of them with a 16-bit
code), any restart interval, 4:4:4, 4:2:2, 4:2:0 and grey.  It can also emit hand-made coefficient blocks (`coefs=`) and
hand-made symbol sequences (`symbols=`), so cases can aim at the walker: a full block with no EOB, ZRL runs, a 16-bit code,
category 15, a stuffed FF 00 as first, middle and last data byte, the inverse DCT's extreme, and the short or wrong streams
behind each status bit.  `tweak=` breaks one header rule at a time for the refusals.

    CASES      every stream that decodes clean (Case.codec: whether a real codec's 16-bit arithmetic can hold it, so that
               Pillow is expected to agree)
    SHORT      (case, the status bits expected somewhere in its words)
    REFUSALS   (name, bytes, a fragment of the InvalidOptionError text)
    FEATURES   what the table as a whole must really contain, by the restatement's own trace
"""
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
SIZES = [(1, 1), (8, 9), (16, 16), (17, 33), (31, 15), (37, 53)]
MODES = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "grey": None}
# H x W whose chroma component is 1, 2 (replicated, as libjpeg does it) or 3 (the narrowest that is filtered) samples wide
NARROW = [(5, 1), (5, 2), (3, 2), (9, 2), (5, 3), (5, 4), (1, 4), (3, 5), (4, 6), (17, 2), (17, 4)]


# ---------------------------------------------------------------- tables
def _dc_table(order):
    """16 categories in `order`: 2 codes of 2 bits, 2 of 3, 3 of 4, 3 of 6, 3 of 8 and 3 of 10, which start with eight 1 bits
    (Kraft sum 0.999: the all-ones code is free)"""
    counts = [0] * 16
    for length, n in ((2, 2), (3, 2), (4, 3), (6, 3), (8, 3), (10, 3)):
        counts[length - 1] = n
    return counts, list(order)


def _ac_table(first, last):
    """all 256 symbols: 4 codes of 3 bits, 8 of 5, 32 of 8, 211 of 12 and one, `last`, of 16 (Kraft sum 0.93)"""
    counts = [0] * 16
    for length, n in ((3, 4), (5, 8), (8, 32), (12, 211), (16, 1)):
        counts[length - 1] = n
    rest = sorted((rs for rs in range(256) if rs not in first and rs != last), key=lambda rs: ((rs >> 4) + 2 * (rs & 15), rs))
    return counts, list(first) + rest + [last]


DC = [_dc_table([2, 3, 1, 4, 0, 5, 6, 7, 8, 9, 10, 12, 13, 11, 14, 15]), _dc_table([1, 2, 0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])]
AC = [_ac_table([0x00, 0x01, 0x02, 0x11, 0x03, 0x04, 0x12, 0x21, 0x31, 0x41, 0x05, 0xF0], 0x71),
      _ac_table([0x00, 0x01, 0x11, 0x02, 0x21, 0x03, 0x12, 0x31, 0xF0, 0x04, 0x41, 0x51], 0x0A)]
LEN16 = (0x71, 0x0A)      # the symbols behind the 16-bit codes


def encoder(table):
    """{symbol: (code, length)} of a (counts, values) table"""
    counts, values = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_tables(quality):
    """(luma, chroma) in natural order, from nothing but a slope: "fine" is all ones, as a codec's quality 100"""
    u, v = np.meshgrid(np.arange(8), np.arange(8))
    base, step = {"fine": (1, 0), "mid": (3, 2), "coarse": (16, 8)}[quality]
    luma = np.clip(base + step * (u + v), 1, 255)
    chroma = np.clip(base + 2 + (step * 3 // 2) * (u + v), 1, 255) if step else luma
    return luma.reshape(64).astype(int).tolist(), chroma.reshape(64).astype(int).tolist()


# ---------------------------------------------------------------- bits
class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, length):
        assert 0 <= value < 1 << length
        self.acc = (self.acc << length) | value
        self.n += length

    def bytes(self, pad=1):
        """whole bytes, padded with 1 bits (or 0 bits), not yet stuffed"""
        fill = -self.n % 8
        acc = (self.acc << fill) | (((1 << fill) - 1) if pad else 0)
        return acc.to_bytes((self.n + fill) // 8, "big") if self.n else b""


def stuff(raw):
    return raw.replace(b"\xff", b"\xff\x00")


def category(v):
    return int(abs(int(v))).bit_length()


def value_bits(v, s):
    return v if v >= 0 else v + (1 << s) - 1


def put_block(bits, zz, pred, dc, ac):
    """one block of 64 coefficients in zigzag order, the usual way: ZRL for runs of 16, EOB unless the last one is set"""
    diff = int(zz[0]) - pred
    s = category(diff)
    bits.put(*dc[s])
    if s:
        bits.put(value_bits(diff, s), s)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            run -= 16
        s = category(v)
        bits.put(*ac[(run << 4) | s])
        bits.put(value_bits(v, s), s)
        run = 0
    if run:
        bits.put(*ac[0x00])
    return int(zz[0])


# ---------------------------------------------------------------- pixels -> coefficients
_T = np.array([[(0.5 if u else np.sqrt(0.125)) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def _pad(p, bh, bw):
    return np.pad(p, ((0, bh * 8 - p.shape[0]), (0, bw * 8 - p.shape[1])), mode="edge")


def _blocks(p, q):
    """(bh, bw, 64) quantised coefficients in natural order of a padded plane"""
    bh, bw = p.shape[0] // 8, p.shape[1] // 8
    b = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.float64) - 128.0
    c = _T @ b @ _T.T
    return np.rint(c.reshape(bh, bw, 64) / np.asarray(q, np.float64)).astype(np.int64)


def picture(h, w, seed):
    """a smooth scene with texture, H x W x 3 RGB uint8"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 5 + y * 3, 255 - x * 4 + y, y * 7 + 40 * np.sin(x / 3.0)], -1)
    return np.clip(base % 256 + rng.integers(-25, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def planes_of(rgb, sampling):
    """component planes (float) at their own sizes: Y, and Cb, Cr box-averaged by the sampling"""
    r, g, b = (rgb[..., i].astype(np.float64) for i in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    if sampling is None:
        return [y]
    cb = -0.168736 * r - 0.331264 * g + 0.5 * b + 128
    cr = 0.5 * r - 0.418688 * g - 0.081312 * b + 128
    hm, vm = sampling
    out = [y]
    for p in (cb, cr):
        p = np.pad(p, ((0, -p.shape[0] % vm), (0, -p.shape[1] % hm)), mode="edge")
        out.append(p.reshape(p.shape[0] // vm, vm, p.shape[1] // hm, hm).mean(axis=(1, 3)))
    return out


# ---------------------------------------------------------------- the file
def _seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def write(h, w, mode="444", dri=1, quality="mid", seed=0, coefs=None, symbols=None, tweak=None):
    """The bytes of one baseline file.  coefs: per component a (bh, bw, 64) integer array in natural order, in place of the
    picture's; symbols: a function (bits, interval index) -> None that writes interval i's data itself (grey only);
    tweak: {rule: value}, see the code."""
    t = dict(tweak or {})
    sampling = MODES[mode]
    hm, vm = sampling or (1, 1)
    mx, my = -(-w // (8 * hm)), -(-h // (8 * vm))
    ql, qc = quant_tables(quality)
    ql, qc = t.get("quant", (ql, qc))
    if coefs is None and symbols is None:
        pl = planes_of(picture(h, w, seed), sampling)
        coefs = [_blocks(_pad(pl[0], my * vm, mx * hm), ql)] + [_blocks(_pad(p, my, mx), qc) for p in pl[1:]]
    nf = 1 if sampling is None else 3
    out = bytearray(b"\xff\xd8")
    if t.get("jfif", True):
        out += _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    if "exif" in t:
        tiff = b"II*\0\x08\0\0\0\x01\0\x12\x01\x03\0\x01\0\0\0" + struct.pack("<HH", t["exif"], 0) + b"\0\0\0\0"
        out += _seg(0xE1, b"Exif\0\0" + tiff + b"\xff\xd8\xff\xda thumbnail bytes \xff\xd9")      # (a fake thumbnail: stepped over)
    if "adobe" in t:
        out += _seg(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([t["adobe"]]))
    pq = t.get("pq", 0)
    for tq, q in ((0, ql), (1, qc))[:1 if nf == 1 else 2]:
        zz = [q[ZIGZAG[k]] for k in range(64)]
        out += _seg(0xDB, bytes([(pq << 4) | tq]) + (struct.pack(">64H", *zz) if pq else bytes(zz)))
    ids = t.get("ids", [1, 2, 3])[:nf]
    samp = t.get("sampling", [(hm, vm), (1, 1), (1, 1)])[:nf]
    tqs = t.get("tq", [0, 1, 1])[:nf]
    nf_written = t.get("nf", nf)
    sof = struct.pack(">BHHB", t.get("precision", 8), h, w, nf_written)
    for c in range(nf_written):
        cc = min(c, nf - 1)
        sof += bytes([ids[cc] if c < nf else 4, (samp[cc][0] << 4) | samp[cc][1], tqs[cc]])
    out += _seg(t.get("sof", 0xC0), sof)
    for (cls, th), tab in (((0, 0), DC[0]), ((1, 0), AC[0]), ((0, 1), DC[1]), ((1, 1), AC[1]))[:2 if nf == 1 else 4]:
        counts, values = t.get("dht", {}).get((cls, th), tab)
        out += _seg(0xC4, bytes([(cls << 4) | th]) + bytes(counts) + bytes(values))
    if dri:
        out += _seg(0xDD, struct.pack(">H", dri))
    sel = t.get("sel", [(0, 0), (1, 1), (1, 1)])[:nf]
    ns = t.get("ns", nf_written)
    sos = bytes([ns])
    for c in range(ns):
        cc = min(c, nf - 1)
        sos += bytes([ids[cc] if c < nf else 4, (sel[cc][0] << 4) | sel[cc][1]])
    out += _seg(0xDA, sos + b"\0\x3f\0")
    n_mcus = mx * my
    step = dri or n_mcus
    n_int = -(-n_mcus // step)
    enc = [(encoder(DC[0]), encoder(AC[0])), (encoder(DC[1]), encoder(AC[1])), (encoder(DC[1]), encoder(AC[1]))]
    for i in range(n_int):
        bits = Bits()
        if symbols is not None:
            symbols(bits, i)
        else:
            pred = [0] * nf
            for mcu in range(i * step, min((i + 1) * step, n_mcus)):
                row, col = divmod(mcu, mx)
                for c in range(nf):
                    ch, cv = (hm, vm) if c == 0 else (1, 1)
                    for by in range(cv):
                        for bx in range(ch):
                            nat = coefs[c][row * cv + by, col * ch + bx]
                            pred[c] = put_block(bits, [nat[ZIGZAG[k]] for k in range(64)], pred[c], *enc[c])
        raw = bits.bytes()
        if t.get("truncate") == i:
            raw = raw[:t.get("keep", len(raw) // 2)]
        out += stuff(raw)
        if i == t.get("fill_at"):
            out += b"\xff"
        if i + 1 < n_int:
            k = i + t.get("rst_shift", 0) if i >= t.get("rst_from", 1 << 30) else i
            out += bytes([0xFF, 0xD0 + k % 8])
    if "extra_intervals" in t:
        for k in range(t["extra_intervals"]):
            out += bytes([0xFF, 0xD0 + (n_int - 1 + k) % 8]) + b"\x00"
    if "second_scan" in t:
        out += _seg(0xDA, sos + b"\0\x3f\0") + b"\x00"
    if t.get("eoi", True):
        out += b"\xff\xd9"
    return bytes(out)


# ---------------------------------------------------------------- the table
class Case:
    def __init__(self, name, codec=True, **kw):
        self.name, self.codec, self.kw = name, codec, kw
        self._data = None

    def data(self):
        if self._data is None:
            self._data = write(**self.kw)
        return self._data

    def write(self, path):
        with open(path, "wb") as fh:
            fh.write(self.data())
        return path

    def __repr__(self):
        return self.name


def _grid(h, w, mode):
    hm, vm = MODES[mode] or (1, 1)
    return -(-w // (8 * hm)), -(-h // (8 * vm))


def _natural(fn):
    """a (1, 1, 64) block in natural order from zigzag position -> value"""
    nat = np.zeros((1, 1, 64), np.int64)
    for k in range(64):
        nat[0, 0, ZIGZAG[k]] = fn(k)
    return nat


def _search(want, seed):
    """a grey 8 x 16 file of two blocks in ONE interval whose unstuffed data bytes have FF where `want` asks"""
    rng = np.random.default_rng(seed)
    for _ in range(20000):
        blocks = np.zeros((1, 2, 64), np.int64)
        for b in range(2):
            n = int(rng.integers(1, 5))        # (few and small: the samples stay where every codec clips alike)
            ks = rng.choice(64, n, replace=False)
            blocks[0, b, [ZIGZAG[k] for k in ks]] = rng.choice([-255, -127, -63, -31, 31, 63, 127, 255, 3, 15, -1, 1], n)
        bits = Bits()
        pred = 0
        for b in range(2):
            pred = put_block(bits, [blocks[0, b, ZIGZAG[k]] for k in range(64)], pred, encoder(DC[0]), encoder(AC[0]))
        raw = bits.bytes()
        if len(raw) >= 4 and want(raw):
            return blocks
    raise AssertionError("no block found")


def _cases():
    cases = []
    for (h, w) in SIZES:
        for mode in MODES:
            mx, my = _grid(h, w, mode)
            cases.append(Case(f"{h}x{w}-{mode}-row", h=h, w=w, mode=mode, dri=mx, seed=h * w))
    for (h, w) in NARROW:
        for mode in ("422", "420"):
            cases.append(Case(f"narrow-{h}x{w}-{mode}", h=h, w=w, mode=mode, dri=1, seed=3 * h + w, quality="fine"))
    # DRI of one MCU, and of 3 MCUs on rows whose MCU count is no multiple of it: intervals that cross rows, a short last one
    for mode in MODES:
        mx, my = _grid(37, 53, mode)
        d = next(d for d in (3, 5, 7) if mx % d and (mx * my) % d)      # (3, but 5 where 12 MCUs would leave no short interval)
        cases.append(Case(f"37x53-{mode}-dri1", h=37, w=53, mode=mode, dri=1, seed=7))
        cases.append(Case(f"37x53-{mode}-dri{d}", h=37, w=53, mode=mode, dri=d, seed=8))
    cases.append(Case("17x33-444-coarse", h=17, w=33, mode="444", dri=2, quality="coarse", seed=9))
    cases.append(Case("17x33-420-fine", h=17, w=33, mode="420", dri=2, quality="fine", seed=10))
    cases.append(Case("31x15-422-fine", h=31, w=15, mode="422", dri=1, quality="fine", seed=11))
    # more than 64 intervals (81 and 90): the marker counter wraps ten times, more than one wavefront's worth
    cases.append(Case("65x70-444-dri1", h=65, w=70, mode="444", dri=1, seed=12))
    cases.append(Case("129x150-420-dri1", h=129, w=150, mode="420", dri=1, seed=13))
    cases.append(Case("exif-orientation", h=8, w=9, mode="444", dri=2, seed=14, tweak={"exif": 6}))
    cases.append(Case("adobe-ycc", h=8, w=9, mode="444", dri=2, seed=14, tweak={"adobe": 1, "jfif": False}))
    cases.append(Case("sof1", h=8, w=9, mode="420", dri=1, seed=15, tweak={"sof": 0xC1}))
    # hand-made blocks (grey, one block a MCU)
    full = _natural(lambda k: (k % 7) - 3 or 1)                      # every coefficient set: no EOB
    cases.append(Case("full-block", h=8, w=8, mode="grey", dri=1, coefs=[full]))
    zrl = np.concatenate([_natural(lambda k: {0: 5, 20: -3, 63: 2}.get(k, 0)), _natural(lambda k: {0: -4, 40: 7}.get(k, 0))], axis=1)
    cases.append(Case("zrl-runs", h=8, w=16, mode="grey", dri=2, coefs=[zrl]))
    len16 = _natural(lambda k: {0: 9, 8: 1}.get(k, 0))               # run 7, size 1: AC[0]'s 16-bit code
    cases.append(Case("len16-code", h=8, w=8, mode="grey", dri=1, coefs=[len16]))
    cat15 = _natural(lambda k: {0: 1000, 3: 32767, 5: -32767, 9: 16384}.get(k, 0))
    cases.append(Case("category-15", codec=False, h=8, w=8, mode="grey", dri=1, coefs=[cat15]))
    dc15 = np.concatenate([_natural(lambda k: 16384 if k == 0 else 0), _natural(lambda k: -16383 if k == 0 else 0)], axis=1)
    cases.append(Case("dc-category-15", codec=False, h=8, w=16, mode="grey", dri=2, coefs=[dc15]))
    for sign, name in ((1, "plus"), (-1, "minus"), (0, "mixed")):
        ext = _natural(lambda k: sign * 32767 if sign else (32767 if (k * 7) % 3 else -32767))
        cases.append(Case(f"idct-extreme-{name}", codec=False, h=8, w=8, mode="grey", dri=1, coefs=[ext],
                          tweak={"quant": ([255] * 64, [255] * 64)}))
    # DC category 11 has a 10-bit code that starts with eight 1 bits: the interval's first data byte is FF
    first = _natural(lambda k: {0: 1030, 1: -2}.get(k, 0))
    cases.append(Case("ff-first", h=8, w=8, mode="grey", dri=1, quality="fine", coefs=[first]))
    cases.append(Case("ff-middle", h=8, w=16, mode="grey", dri=2, quality="fine", coefs=[_search(lambda r: 0xFF in r[1:-1] and r[0] != 0xFF and r[-1] != 0xFF, 2)]))
    cases.append(Case("ff-last", h=8, w=16, mode="grey", dri=2, quality="fine", coefs=[_search(lambda r: r[-1] == 0xFF and 0xFF not in r[:-1], 3)]))
    return cases


def _short():
    dc, ac = encoder(DC[0]), encoder(AC[0])

    def nocode(bits, i):            # DC 0, then 16 one-bits where an AC code is expected: symbol 0, the end of the block
        bits.put(*dc[0])
        bits.put(0xFFFF, 16)

    def dc_nocode(bits, i):         # 16 one-bits where the DC code is expected, then EOB
        bits.put(0xFFFF, 16)
        bits.put(*ac[0x00])

    def zrl_run(bits, i):           # four ZRLs from k = 1: 17, 33, 49, 65
        bits.put(*dc[0])
        for _ in range(4):
            bits.put(*ac[0xF0])

    def coef_run(bits, i):          # a coefficient at 60, then a run of 5 and a value: k = 66
        bits.put(*dc[2])
        bits.put(3, 2)
        for _ in range(3):
            bits.put(*ac[0xF0])
        bits.put(*ac[0xB1])         # k = 1 + 48 + 11 = 60
        bits.put(1, 1)
        bits.put(*ac[0x52])         # k = 61 + 5 = 66: dropped
        bits.put(2, 2)

    short = [(Case("short-nocode", codec=False, h=8, w=8, mode="grey", dri=1, symbols=nocode), 1),
             (Case("short-dc-nocode", codec=False, h=8, w=8, mode="grey", dri=1, symbols=dc_nocode), 1),
             (Case("short-zrl-run", codec=False, h=8, w=8, mode="grey", dri=1, symbols=zrl_run), 4),
             (Case("short-coef-run", codec=False, h=8, w=8, mode="grey", dri=1, symbols=coef_run), 4),
             (Case("short-empty-interval", codec=False, h=8, w=24, mode="grey", dri=1, symbols=lambda b, i: None if i == 1 else clean_block(b)), 2),
             (Case("short-truncated", codec=False, h=37, w=53, mode="420", dri=4, seed=21, tweak={"truncate": 2}), 2),
             (Case("short-truncated-to-nothing", codec=False, h=17, w=33, mode="444", dri=3, seed=22, tweak={"truncate": 0, "keep": 0}), 2)]
    return short


def clean_block(bits):
    """a clean DC-only block"""
    bits.put(*encoder(DC[0])[1])
    bits.put(1, 1)
    bits.put(*encoder(AC[0])[0x00])


def _refusals():
    ok = dict(h=17, w=33, mode="420", dri=2, seed=5)
    grey = dict(h=8, w=16, mode="grey", dri=1, seed=5)

    def f(tweak, base=ok, **kw):
        return write(**{**base, **kw, "tweak": tweak})
    over = ([3] + [0] * 15, [0, 1, 2])
    many = ([0] * 7 + [255, 2] + [0] * 7, list(range(256)) + [0])
    return [
        ("progressive", f({"sof": 0xC2}), "SOF2 (progressive DCT)"),
        ("lossless", f({"sof": 0xC3}), "SOF3 (lossless)"),
        ("arithmetic", f({"sof": 0xC9}), "SOF9 (arithmetic coding)"),
        ("arithmetic-progressive", f({"sof": 0xCA}), "SOF10 (arithmetic coding, progressive)"),
        ("precision-12", f({"precision": 12}), "SOF0 precision = 12"),
        ("sof1-precision-12", f({"precision": 12, "sof": 0xC1}), "SOF1 precision = 12"),
        ("several-scans", f({"second_scan": True}), "several scans"),
        ("scan-of-one-component", f({"ns": 1}), "SOS Ns = 1"),
        ("nf-2", f({"nf": 2}), "SOF0 Nf = 2"),
        ("nf-4", f({"nf": 4}), "SOF0 Nf = 4"),
        ("sampling-1x2", f({"sampling": [(1, 2), (1, 1), (1, 1)]}, mode="444"), "SOF sampling = [(1, 2), (1, 1), (1, 1)]"),
        ("sampling-4x1", f({"sampling": [(4, 1), (1, 1), (1, 1)]}, mode="444"), "SOF sampling = [(4, 1), (1, 1), (1, 1)]"),
        ("sampling-chroma", f({"sampling": [(2, 2), (2, 1), (1, 1)]}), "SOF sampling = [(2, 2), (2, 1), (1, 1)]"),
        ("pq-1", f({"pq": 1}), "DQT Pq = 1"),
        ("no-quant-table", f({"tq": [0, 2, 2]}), "SOF Tq = 2"),
        ("no-dc-table", f({"sel": [(1, 0)]}, base=grey), "SOS Td = 1"),
        ("no-ac-table", f({"sel": [(0, 1)]}, base=grey), "SOS Ta = 1"),
        ("selector-2", f({"sel": [(0, 0), (2, 1), (1, 1)]}), "SOS Td = 2"),
        ("dht-overflow", f({"dht": {(0, 0): over}}), "the counts overflow the code space"),
        ("dht-257-values", f({"dht": {(1, 0): many}}), "DHT = 257 values"),
        ("adobe-transform-0", f({"adobe": 0, "jfif": False}), "APP14 Adobe transform = 0"),
        ("adobe-transform-2", f({"adobe": 2, "jfif": False}), "APP14 Adobe transform = 2"),
        ("ids-rgb", f({"ids": [82, 71, 66], "jfif": False}), "SOF component ids = 'R', 'G', 'B'"),
        ("no-restart-interval", f({}, dri=0), "DRI = none: "),
        ("restart-interval-too-long", f({}, dri=8193), "DRI = 8193: "),
        ("eoi-before-the-scan", f({})[:20] + b"\xff\xd9", "EOI = byte 20"),
        ("rst-out-of-sequence", f({"rst_from": 1, "rst_shift": 1}), "restart markers out of sequence: RST1 is expected"),
        ("interval-count", f({"extra_intervals": 1}), "restart intervals = "),
        ("fill-byte", f({"fill_at": 1}), "fill byte = FF FF at byte"),
        ("no-eoi", f({"eoi": False}), "EOI = none"),
    ]


CASES = _cases()
SHORT = _short()
REFUSALS = _refusals()
FEATURES = {"zrl", "len16", "cat15", "dc-cat15", "noeob", "ff-first", "ff-middle", "ff-last"}


def pillow_files():
    """(name, bytes) of the same pictures written by Pillow, for the pin; empty without Pillow"""
    try:
        from PIL import Image
    except ImportError:
        return []
    import io
    out = []
    for (h, w) in SIZES:
        rgb = picture(h, w, h + w)
        for sub, mode in ((0, "444"), (1, "422"), (2, "420"), (None, "grey")):
            for q in (30, 90, 100):
                for kw in ({"restart_marker_rows": 1}, {"restart_marker_blocks": 3}, {"restart_marker_blocks": 1, "optimize": True}):
                    im = Image.fromarray(rgb if sub is not None else rgb[:, :, 1])
                    b = io.BytesIO()
                    im.save(b, "JPEG", quality=q, **({} if sub is None else {"subsampling": sub}), **kw)
                    out.append((f"pil-{h}x{w}-{mode}-q{q}-{'-'.join(kw)}", b.getvalue()))
    for (h, w) in NARROW:
        rgb = picture(h, w, 7 * h + w)
        for sub, mode in ((1, "422"), (2, "420")):
            b = io.BytesIO()
            Image.fromarray(rgb).save(b, "JPEG", quality=95, subsampling=sub, restart_marker_rows=1)
            out.append((f"pil-narrow-{h}x{w}-{mode}", b.getvalue()))
    return out
