"""CPU: the restatement of raw_ljpeg (tests/ljpeg_restatement.py) decodes the two hand-computed known answers, inverts the
independent encoder of tests/ljpeg_cases.py on every case, and the case table means something: every kernel path `paths`
names is reached by some case and every case reaches one."""
import numpy as np
import pytest

import ljpeg_cases as LC
import ljpeg_restatement as R


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """{case name: what the writer returned} of the whole table, short streams included"""
    d = tmp_path_factory.mktemp("ljpeg")
    return {c.name: c.write(str(d / (c.name + ".dng"))) for c in LC.CASES + [s[0] for s in LC.SHORT]}


@pytest.mark.parametrize("known", LC.KNOWN, ids=["46-bits", "stuffed-FF"])
def test_known_answers(known):
    got, status = R.decode(known["data"], [LC.KNOWN_TABLE] * 2, known["precision"], known["lines"], known["x"], known["ncomp"],
                           known["predictor"])
    assert status == 0
    assert got.tolist() == known["want"]
    # with EOI behind the data, as it lies in a file: the marker ends the data
    got, status = R.decode(known["data"] + b"\xff\xd9", [LC.KNOWN_TABLE] * 2, known["precision"], known["lines"], known["x"],
                           known["ncomp"], known["predictor"])
    assert status == 0 and got.tolist() == known["want"]
    # one byte short: the last sample needs bits from beyond the end
    _, status = R.decode(known["data"][:-1], [LC.KNOWN_TABLE] * 2, known["precision"], known["lines"], known["x"], known["ncomp"],
                         known["predictor"])
    assert status == R.OVERRUN


def test_the_first_known_answer_takes_46_bits():
    k = LC.KNOWN[0]
    stream, info = LC.encode(np.array(k["want"]), 2, 1, 12, tables=LC.KNOWN_TABLE)
    assert stream[info["scan_off"]:info["scan_off"] + info["data_bytes"]] == k["data"]
    stream, info = LC.encode(np.array(LC.KNOWN[1]["want"]), 2, 1, 12, tables=LC.KNOWN_TABLE)
    assert stream[info["scan_off"]:info["scan_off"] + info["data_bytes"]] == LC.KNOWN[1]["data"] and info["stuffed"] == 1


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_the_restatement_inverts_the_encoder(written, case):
    info = written[case.name]
    tiled, seg_h, seg_w = case.segments()
    nsx = -(-case.w // seg_w)
    stored = case.stored()
    for k, stream in enumerate(info["streams"]):
        got, status = R.decode_stream(stream)
        assert status == 0, (case, k)
        y0, x0 = (k // nsx) * seg_h, (k % nsx) * seg_w
        want = stored[y0:y0 + seg_h, x0:x0 + seg_w]
        assert np.array_equal(got[:want.shape[0], :want.shape[1]], want), (case, k)
        p = R.parse(stream)
        assert (p["precision"], p["ncomp"], p["predictor"], p["al"]) == (case.precision, case.ncomp, case.predictor, 0)
        assert p["x"] * p["ncomp"] == seg_w and p["scan_off"] == info["infos"][k]["scan_off"]
        assert [list(map(list, t)) for t in p["tables"]] == [list(map(list, t)) for t in info["infos"][k]["tables"]]


@pytest.mark.parametrize("short", LC.SHORT, ids=lambda s: repr(s[0]))
def test_short_streams_have_their_status(written, short):
    case, flagged, flag = short
    info = written[case.name]
    _, seg_h, _ = case.segments()
    for k, stream in enumerate(info["streams"]):
        got, status = R.decode_stream(stream)
        if k == flagged:
            assert status & flag, (case, status)
        else:
            assert status == 0 and np.array_equal(got, case.stored()[k * seg_h:(k + 1) * seg_h])


def test_every_path_is_reached_and_no_case_is_vacuous(written):
    reached = {}
    for c in LC.CASES:
        seen = LC.paths(c, written[c.name])
        assert seen and seen <= set(LC.PATHS), (c, seen)
        for p in seen:
            reached.setdefault(p, []).append(c.name)
    assert set(reached) == set(LC.PATHS), set(LC.PATHS) - set(reached)
    long = written["16bit-64x130-random-long-stream"]["infos"][0]
    assert long["data_bytes"] >= 3 * LC.RING >= 3 * LC.CHUNK       # crosses every staging boundary at least three times
    assert written["16bit-long-codes"]["infos"][0]["longest"] == 16
    tables = [i["tables"] for i in written["12bit-tiles-21x37-shuffled"]["infos"]]
    assert len({repr(t) for t in tables}) > 1                       # a different optimal table in the tiles
