"""The case table of the split lossless-JPEG decoder (csrc/kernels_ljpeg_split.hpp), shared by test_ljpeg_split_host.py,
test_ljpeg_split_core_host.py (CPU) and test_gpu_ljpeg_split.py (GPU): every case of tests/ljpeg_cases.py, short streams
included, and a few long ones, each the smallest that reaches its path.  `paths` predicts what a case exercises.

Shapes, against the kernels' geometry: the lanes are the segments' subsequences of sub_bytes bytes, counted segment after
segment, GROUP = 256 to a workgroup -- 2 KB of data a group at sub_bytes 8, 32 KB at the default 128; predictor 1 is a scan down
the first columns and then one wave per row in chunks of ROW_CHUNK = 512 samples with a carry; predictors 2 to 7 are one wave
per segment.
"""
import numpy as np

import ljpeg_cases as LC
import ljpeg_split_restatement as S

GROUP, ROW_CHUNK = 256, 512         # split::GROUP of csrc/kernels_split_common.hpp, ljpeg::ROW_CHUNK of csrc/kernels_ljpeg_split.hpp
SUBS = (8, 128)

# one-code tables of different lengths: component 0 "0", component 1 "00", both category 0
ONE_BIT, TWO_BITS = ([1] + [0] * 15, [0]), ([0, 1] + [0] * 14, [0])


def _ordinary(k, stream, info):
    """the second strip of NEVER_BESIDE: two rows of random samples under their own optimal tables"""
    if k != 1:
        return stream
    rng = np.random.default_rng(77)
    return LC.encode(rng.integers(0, 4096, size=(2, 920)), 2, 1, 12)[0]


# 128 x 256 random 16-bit samples: 65 769 bytes of data, three groups at the default sub_bytes (127 rows give 65 265)
LONG_128 = LC.Case("16bit-128x256-random-three-groups-at-128", 128, 256, 16, ncomp=2)
# every sample the mid value: all differences 0, three zero bits a pixel, 4140 bytes, three groups at sub_bytes 8.  A cold
# lane's phase never falls into step (every phase of an all-zero stream decodes without complaint): the case that needs every
# round.  A valid file, the kind a flat dark frame gives.
NEVER = LC.Case("12bit-24x920-never-synchronises", 24, 920, 12, ncomp=2, fill="mid", tables=[ONE_BIT, TWO_BITS])
# the same strip with an ordinary one of two rows behind it in the same span (its `expected` does not hold for that strip)
NEVER_BESIDE = LC.Case("12bit-26x920-never-synchronises-beside-ordinary", 26, 920, 12, ncomp=2, fill="mid", tables=[ONE_BIT, TWO_BITS],
                       rows_per_strip=24, mangle=_ordinary)


class Given(LC.Case):
    """a case whose stored samples are given"""

    def __init__(self, name, samples, bits, **kw):
        samples = np.array(samples, np.int64)
        samples.setflags(write=False)
        super().__init__(name, samples.shape[0], samples.shape[1], bits, **kw)
        self._samples = samples

    def stored(self):
        return self._samples


def _odd_flip(rows, cols):
    """the `flip` fill behind one byte that is not FF: the first pixel's differences are 1 and 2 (under LONG_TABLE "10" "1" and
    "110" "10": the byte BA), every other difference is 32768 (FF 00 FF 00): the stuffed 00s lie at the even offsets, where
    subsequences start"""
    a = np.zeros((rows, cols), np.int64)
    a[0, 0::2] = np.where(np.arange(cols // 2) % 2 == 0, 32769, 1)
    a[0, 1::2] = np.where(np.arange(cols // 2) % 2 == 0, 32770, 2)
    for r in range(1, rows):
        a[r] = a[r - 1] ^ 32768
    return a


STUFFED_STARTS = Given("16bit-3x140-stuffed-00-at-subsequence-starts", _odd_flip(3, 140), 16, ncomp=2, tables=LC.LONG_TABLE)
LONG = [LONG_128, NEVER, STUFFED_STARTS]
SHORT = LC.SHORT
WHOLE = LC.CASES + LONG                                  # `expected()` holds
ALL = WHOLE + [s[0] for s in SHORT] + [NEVER_BESIDE]
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)

PATHS = ("rounds-0", "rounds-1", "rounds-more", "group-spanning", "segment-starts-mid-group", "segment-ends-mid-group", "pass-through",
         "surplus-symbols", "stuffed-at-a-subsequence-start", "column-seed", "row-carry", "per-segment-predict", "one-component",
         "two-components", "several-segments")


def paths(case, segs, sub):
    """The paths of the split decoder a case reaches at sub_bytes `sub` (`segs`: ljpeg_split_restatement.segments_of its file):
      rounds-0 / rounds-1 / rounds-more   the rounds behind round 0 until every exit is the true one
      group-spanning                  a segment whose lanes lie in more than one workgroup
      segment-starts-mid-group, segment-ends-mid-group   ... whose first lane is not a group's first / last lane not its last
      pass-through                    a lane that decodes nothing: its entry is END (or lies behind its subsequence)
      surplus-symbols                 symbols behind the quota: the padding bits decode as further ones, and are dropped
      stuffed-at-a-subsequence-start  a subsequence whose first byte is a stuffed 00: its cold state starts one byte later
      column-seed                     predictor 1 on more than one row: the scan down the first columns
      row-carry                       predictor 1 on a row of more than ROW_CHUNK samples
      per-segment-predict             predictors 2 to 7: one wave per segment
      one-component, two-components, several-segments"""
    r = S.rounds_needed(segs, sub, GROUP)
    seen = {"rounds-0" if r == 0 else "rounds-1" if r == 1 else "rounds-more"}
    if len(segs) > 1:
        seen.add("several-segments")
    at = 0
    for seg in segs:
        subs = S.subsequences(len(seg.data.raw), sub)
        first, last = at, at + len(subs) - 1
        at += len(subs)
        if first // GROUP != last // GROUP:
            seen.add("group-spanning")
        if first % GROUP:
            seen.add("segment-starts-mid-group")
        if last % GROUP != GROUP - 1:
            seen.add("segment-ends-mid-group")
        if any(S.cold(seg, lo)[0] != lo for lo, _ in subs):
            seen.add("stuffed-at-a-subsequence-start")
        seen.add("one-component" if seg.ncomp == 1 else "two-components")
        if seg.predictor == 1:
            if seg.rows > 1:
                seen.add("column-seed")
            if seg.cols > ROW_CHUNK:
                seen.add("row-carry")
        else:
            seen.add("per-segment-predict")
    if S.pass_through_lanes(segs, sub):
        seen.add("pass-through")
    total = {}
    for (seg, lo, hi, last), (_, (_, n)) in zip(S.lanes_of(segs, sub), S.exits(segs, sub)):
        total[id(seg)] = total.get(id(seg), 0) + n
    if any(total[id(seg)] > seg.quota for seg in segs):
        seen.add("surplus-symbols")
    return seen


MUTATED = ("12bit-tiles-21x37-shuffled", "14bit-tiles-21x37-p6", "16bit-flip-32768-all-stuffed", "12bit-3x530-p2", "16bit-long-codes",
           "12bit-known-table-fill-ff", "12bit-crop-2-4-strips")


def mutants(span, layout, rng, n=10):
    """n seeded corruptions of a span (bytes), taken from the bytes of its segments' data only: headers, gaps and the
    descriptors read from them stay"""
    segs = [(int(s["scan_off"]), int(s["scan_off"]) + int(s["scan_bytes"])) for s in layout.segments]
    out = []
    for k in range(n):
        m = bytearray(span)
        for _ in range(1 + k % 4):
            lo, hi = segs[int(rng.integers(len(segs)))]
            m[int(rng.integers(lo, hi))] = int(rng.choice([0x00, 0xFF, 0xD0, 0x7F, int(rng.integers(256))]))
        out.append(bytes(m))
    return out
