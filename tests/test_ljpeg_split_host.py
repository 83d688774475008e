"""CPU: the split lossless-JPEG decoder's definition (tests/ljpeg_split_restatement.py) against the serial one
(tests/ljpeg_restatement.py) and against the samples the writer stored, on every case of tests/ljpeg_split_cases.py and on
seeded corruptions; every path the case table names is reached by some case; and the rounds the cases need."""
import numpy as np
import pytest

import ljpeg_cases as LC
import ljpeg_restatement as R
import ljpeg_split_cases as SC
import ljpeg_split_restatement as S
from shinestacker_amd import dng


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """{case name: (DngFrame, its Segments, what write_dng returned)}"""
    d = tmp_path_factory.mktemp("ljpeg_split")
    out = {}
    for c in SC.ALL:
        info = c.write(str(d / (c.name + ".dng")))
        frame = dng.read(str(d / (c.name + ".dng")))
        out[c.name] = (frame, S.segments_of(frame.span, frame.layout), info)
    return out


@pytest.fixture(scope="module")
def reached(written):
    return {(c.name, sub): SC.paths(c, written[c.name][1], sub) for c in SC.ALL for sub in SC.SUBS}


def test_no_case_is_vacuous(reached):
    seen = set().union(*reached.values())
    assert seen == set(SC.PATHS), set(SC.PATHS) ^ seen


def test_the_long_cases_reach_what_they_were_made_for(written, reached):
    _, segs, info = written[SC.LONG_128.name]
    assert info["infos"][0]["data_bytes"] > 65536 and S.groups_touched(segs, 128) == 3
    assert {"group-spanning", "segment-ends-mid-group"} <= reached[(SC.LONG_128.name, 128)]
    _, segs, _ = written[SC.NEVER.name]
    assert S.groups_touched(segs, 8) == 3 and "rounds-more" in reached[(SC.NEVER.name, 8)]
    assert "group-spanning" in reached[("16bit-64x130-random-long-stream", 8)]
    # (the flip cases' FF 00 pairs start at the data's first byte, at an even and an odd place of the span: every subsequence
    # starts on an FF; behind one other byte the 00s stand at the subsequence starts)
    for sub in SC.SUBS:
        assert "stuffed-at-a-subsequence-start" in reached[(SC.STUFFED_STARTS.name, sub)]
        for name in ("16bit-flip-32768-all-stuffed", "16bit-flip-32768-all-stuffed-odd-start"):
            assert "stuffed-at-a-subsequence-start" not in reached[(name, sub)]
    assert "segment-starts-mid-group" in reached[("12bit-tiles-21x37-shuffled", 8)]
    assert "row-carry" in reached[("12bit-2x24580-wider-than-the-line-buffer", 128)]
    _, segs, _ = written[SC.NEVER_BESIDE.name]
    assert [S.differences(s)[1] for s in segs] == [0, 0] and segs[1].data.nreal > 2048


def test_the_rounds_the_cases_need(written):
    """The never-synchronising case needs every round, groups - 1 (2 at sub_bytes 8).  Ordinary cases need none or one at the
    default sub_bytes, every one of them.  At sub_bytes 8, which the tests use to reach several groups with small files, that
    does not hold for all, and no state of (bit position, component) can make it hold: a lane of 8 bytes holds three samples
    of random 16-bit data, whose 15 or 16 random extra bits a cold walk cannot fall into step with, and with two components a
    cold walk that found the bit position has the component right half of the time -- a run of groups that start on the wrong
    one is repaired a group a round.  Counted: 16bit-64x130-random 8 rounds over 9 groups, 16bit-128x256-random 31 over 33,
    12bit-2x24576-p2 (random) 32 over 39, 12bit-2x24580 (smooth) 3 over 4; every other ordinary case 0 or 1.  There the bound
    groups - 1, which the host forms enqueue, is what is asserted."""
    for sub in SC.SUBS:
        for c in SC.ALL:
            segs = written[c.name][1]
            r = S.rounds_needed(segs, sub)
            assert r <= S.groups_touched(segs, sub) - 1, (c, sub)
            if c in (SC.NEVER, SC.NEVER_BESIDE) and sub == 8:
                assert r == S.groups_touched(segs[:1], sub) - 1 == 2, (c, r)
            elif sub == 128:
                assert r <= 1, (c, sub, r)


@pytest.mark.parametrize("case", LC.CASES + [s[0] for s in SC.SHORT], ids=repr)
def test_the_split_restatement_equals_the_serial_one(case, written):
    frame, segs, _ = written[case.name]
    want, status = R.unpack_layout(frame.span, frame.layout)
    got, st, _ = S.unpack_layout(frame.span, frame.layout)
    assert st.tolist() == status.tolist()
    if not status.any():
        assert np.array_equal(got, want)
        if case in LC.CASES:
            assert np.array_equal(got, case.expected())
    for k, seg in enumerate(segs):          # segment by segment, the flagged ones left out
        s = frame.layout.segments[k]
        data = bytes(frame.span)[int(s["scan_off"]):int(s["scan_off"]) + int(s["scan_bytes"])]
        tables = [(s["counts"][c].tolist(), s["values"][c].tolist()) for c in range(seg.ncomp)]
        vals, flag = R.decode(data, tables, seg.precision, seg.rows, seg.cols // seg.ncomp, seg.ncomp, seg.predictor)
        mine, mflag = S.decode(seg)
        assert mflag == flag and (flag or np.array_equal(mine, vals)), (case, k)


@pytest.mark.parametrize("case", SC.LONG, ids=repr)
def test_the_long_cases_return_the_stored_samples(case, written):
    """(the serial restatement's reader is quadratic in the stream's length: the writer's own samples stand in for it)"""
    frame, _, _ = written[case.name]
    got, st, _ = S.unpack_layout(frame.span, frame.layout)
    assert not st.any() and np.array_equal(got, case.expected())


def test_seeded_mutants_agree_on_what_is_unflagged(written):
    rng = np.random.default_rng(2026)
    flagged = clean = 0
    for name in SC.MUTATED:
        frame, _, _ = written[name]
        lay = frame.layout
        for m in SC.mutants(bytes(frame.span), lay, rng):
            for k, seg in enumerate(S.segments_of(np.frombuffer(m, np.uint8), lay)):
                s = lay.segments[k]
                data = m[int(s["scan_off"]):int(s["scan_off"]) + int(s["scan_bytes"])]
                tables = [(s["counts"][c].tolist(), s["values"][c].tolist()) for c in range(seg.ncomp)]
                vals, flag = R.decode(data, tables, seg.precision, seg.rows, seg.cols // seg.ncomp, seg.ncomp, seg.predictor)
                mine, mflag = S.decode(seg)
                assert (mflag == 0) == (flag == 0), (name, k)
                if not flag:
                    assert np.array_equal(mine, vals), (name, k)
                flagged += flag != 0
                clean += flag == 0
    assert flagged > 10 and clean > 10
