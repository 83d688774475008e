"""The case table of the split JPEG decoder's tests, written by tests/jpeg_cases.py's independent writer.

    PLAIN     clean files WITHOUT a restart interval (dri=0): every size x mode, every narrow shape, the hand-made blocks
              (full block, ZRL, 16-bit code, category 15, FF first, middle and last), a subsequence that begins on a stuffed
              00, and the two dense 129 x 150 pictures at quality "fine" whose cold starts join the true decode slowly
    SLOW      the names of those two
    LONG      a DRI of 8193, above jpeg.MAX_DRI
    ALWAYS    files WITH restart intervals for read(split="always")
    SHORT     (case, status bits expected) -- jpeg_cases.SHORT in one piece, and a stream of FF 00 pairs
    FEATURES  what the table must really contain (tests/test_jpeg_split_host.py checks each)
"""
import jpeg_cases as JC
from jpeg_cases import Case

HANDMADE = ("full-block", "zrl-runs", "len16-code", "category-15", "dc-category-15", "ff-first", "ff-middle", "ff-last")
SLOW = ("129x150-444-fine", "129x150-420-fine")


def _plain():
    out = []
    for (h, w) in JC.SIZES:
        for mode in JC.MODES:
            out.append(Case(f"{h}x{w}-{mode}", h=h, w=w, mode=mode, dri=0, seed=h * w + 1))
    for (h, w) in JC.NARROW:
        for mode in ("422", "420"):
            out.append(Case(f"narrow-{h}x{w}-{mode}", h=h, w=w, mode=mode, dri=0, seed=3 * h + w, quality="fine"))
    by_name = {c.name: c for c in JC.CASES}
    for name in HANDMADE:
        c = by_name[name]
        out.append(Case(name, codec=c.codec, **{**c.kw, "dri": 0}))
    out.append(_stuffed_at_a_start())
    out.append(Case(SLOW[0], h=129, w=150, mode="444", dri=0, quality="fine", seed=31))
    out.append(Case(SLOW[1], h=129, w=150, mode="420", dri=0, quality="fine", seed=31))
    return out


def scan_of(data):
    """the bytes of the scan of a file of the writer's: behind the SOS segment, in front of EOI"""
    at = data.index(b"\xff\xda")
    n = (data[at + 2] << 8) | data[at + 3]
    return data[at + 2 + n:-2] if data[-2:] == b"\xff\xd9" else data[at + 2 + n:]


def stuffed_starts(scan, sub_bytes):
    """the subsequences of a scan in one piece that begin on the 00 of an FF 00 pair"""
    return [j for j in range(1, -(-len(scan) // sub_bytes)) if scan[j * sub_bytes - 1] == 0xFF and scan[j * sub_bytes] == 0]


def _stuffed_at_a_start():
    for seed in range(400):
        kw = dict(h=17, w=33, mode="444", dri=0, quality="fine", seed=1000 + seed)
        if stuffed_starts(scan_of(JC.write(**kw)), 8):
            return Case("stuffed-00-first", **kw)
    raise AssertionError("no picture found")


def _ones(bits, i):
    """FF 00 pairs: 16 one-bits match no code, so DC and AC symbols of 16 bits each, all the way"""
    for _ in range(40):
        bits.put(0xFFFF, 16)


def _short():
    out = []
    for case, want in JC.SHORT:
        kw = {**case.kw, "dri": 0}
        if "tweak" in kw and "truncate" in kw["tweak"]:
            kw["tweak"] = {**kw["tweak"], "truncate": 0}
        out.append((Case(case.name, codec=False, **kw), want))
    out.append((Case("ff00-pairs", codec=False, h=8, w=16, mode="grey", dri=0, symbols=_ones), 1))
    return out


PLAIN = _plain()
LONG = [Case("17x33-420-dri8193", h=17, w=33, mode="420", dri=8193, seed=5),
        Case("65x70-444-dri8193", h=65, w=70, mode="444", dri=8193, seed=6)]
ALWAYS = [c for c in JC.CASES if c.name.startswith("37x53-") and "-dri" in c.name or c.name == "129x150-420-dri1"]
SHORT = _short()
FEATURES = set(JC.FEATURES)
