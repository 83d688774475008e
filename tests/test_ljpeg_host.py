"""CPU: dng.read on lossless-JPEG DNGs against the independent writer of tests/ljpeg_cases.py -- layout, one descriptor per
segment, the span; the restatement run on those descriptors returns the samples the writer stored; every new refusal by name
and value; the three short-stream statuses; and an uncompressed file parses exactly as before."""
import struct

import numpy as np
import pytest

import dng_cases as DC
import ljpeg_cases as LC
import ljpeg_restatement as R
from shinestacker_amd import _lib, dng
from shinestacker_amd.errors import InvalidOptionError


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    d = tmp_path_factory.mktemp("ljpeg")
    out = {}
    for c in LC.CASES + [s[0] for s in LC.SHORT]:
        info = c.write(str(d / (c.name + ".dng")))
        out[c.name] = (dng.read(str(d / (c.name + ".dng"))), info)
    return out


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_parser_returns_the_writers_layout_descriptors_and_span(case, written):
    frame, info = written[case.name]
    lay = frame.layout
    tiled, seg_h, seg_w = case.segments()
    top, left, ch, cw = case.crop()
    assert lay.compression == 7 and (lay.bits, lay.big_endian) == (case.bits, case.kw.get("e", "<") == ">")
    assert (lay.image_height, lay.image_width) == (case.h, case.w)
    assert (lay.tiled, lay.seg_height, lay.seg_width) == (tiled, seg_h, seg_w)
    assert (lay.crop_y, lay.crop_x, lay.height, lay.width) == (top, left, ch, cw)
    assert frame.shape == (ch, cw) and frame.dtype == lay.dtype == case.dtype and lay.shift == case.shift()
    offs = np.array(info["offsets"])
    sizes = np.array([len(s) for s in info["streams"]])
    assert [lay.segment_bytes(k) for k in range(len(offs))] == sizes.tolist()          # the file's byte counts
    assert lay.offsets.tolist() == (offs - offs.min()).tolist()
    assert frame.span.nbytes == (offs + sizes).max() - offs.min()
    with open(frame.path, "rb") as fh:
        data = fh.read()
    assert bytes(frame.span) == data[offs.min():(offs + sizes).max()]
    segs = lay.segments
    assert segs.dtype == _lib.LJPEG_SEG_DTYPE and segs.dtype.itemsize == 96 and len(segs) == len(offs)
    for k, (s, i) in enumerate(zip(segs, info["infos"])):
        rows = seg_h if tiled else min(seg_h, case.h - (k // lay.grid[1]) * seg_h)
        assert (s["ncomp"], s["predictor"], s["precision"]) == (case.ncomp, case.predictor, case.precision)
        assert (s["x"] * s["ncomp"], s["y"]) == (seg_w, rows)
        assert s["scan_off"] == offs[k] - offs.min() + i["scan_off"]
        assert s["scan_bytes"] == sizes[k] - i["scan_off"]          # the data runs to the segment's end: EOI ends it
        for c, (counts, values) in enumerate(i["tables"]):
            assert s["counts"][c].tolist() == list(counts)
            assert s["values"][c].tolist() == list(values) + [0] * (17 - len(values))
        assert not s["pad"].any() and s["reserved"] == 0


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_restatement_on_the_parsed_descriptors_returns_the_stored_samples(case, written):
    frame, _ = written[case.name]
    got, status = R.unpack_layout(frame.span, frame.layout)
    assert not status.any()
    assert got.dtype == case.dtype and np.array_equal(got, case.expected())


@pytest.mark.parametrize("short", LC.SHORT, ids=lambda s: repr(s[0]))
def test_short_streams_parse_and_carry_their_status(short, written):
    case, flagged, flag = short
    frame, _ = written[case.name]
    got, status = R.unpack_layout(frame.span, frame.layout)
    assert status[flagged] & flag and not np.delete(status, flagged).any()
    _, seg_h, _ = case.segments()
    keep = np.ones(case.h, bool)
    keep[flagged * seg_h:(flagged + 1) * seg_h] = False
    assert np.array_equal(got[keep], case.expected()[keep])


# ------------------------------------------------------------------------------------------------ refusals
def _patch(find, put, nth=0):
    """mangle: in segment 1's stream replace the nth occurrence of `find` (in front of the data) by `put`"""
    def mangle(k, stream, info):
        if k != 1:
            return stream
        head = stream[:info["scan_off"]]
        at = -1
        for _ in range(nth + 1):
            at = head.index(find, at + 1)
        return head[:at] + put + head[at + len(find):] + stream[info["scan_off"]:]
    return mangle


def _sof(ncomp=2, precision=12, lines=3, x=9, marker=0xC3):
    return bytes([0xFF, marker]) + struct.pack(">HBHHB", 8 + 3 * ncomp, precision, lines, x, ncomp)


SOF3 = _sof()
SOS = b"\xff\xda" + struct.pack(">HB", 10, 2) + bytes([1, 0x00, 2, 0x10])
BAD_COUNTS = bytes([3] + [0] * 15)          # three codes of one bit
REFUSALS = [
    ("no-soi", _patch(b"\xff\xd8", b"\xff\xd9"), ("does not start with SOI", "FF D9")),
    ("sof0", _patch(SOF3, _sof(marker=0xC0)), ("SOF0 baseline DCT",)),
    ("sof11", _patch(SOF3, _sof(marker=0xCB)), ("SOF11 arithmetic lossless",)),
    ("dri", _patch(SOF3, b"\xff\xdd\x00\x04\x00\x08" + SOF3), ("DRI", "restart interval of 8")),
    ("nf-4", _patch(SOF3 + bytes([1, 0x11, 0, 2, 0x11, 0]), _sof(ncomp=4, x=4) + bytes([1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0, 4, 0x11, 0])),
     ("Nf = 4 components",)),
    ("frame-lines", _patch(SOF3, _sof(lines=4)), ("a frame of 4 lines of 9 x 2 samples does not match its segment of 3 x 18",)),
    ("frame-x", _patch(SOF3, _sof(x=8)), ("a frame of 3 lines of 8 x 2 samples does not match its segment of 3 x 18",)),
    ("precision", _patch(SOF3, _sof(precision=14)), ("P = 14", "BitsPerSample = 12")),
    ("al", _patch(SOS + bytes([1, 0, 0]), SOS + bytes([1, 0, 2])), ("Al = 2",)),
    ("predictor-0", _patch(SOS + bytes([1, 0, 0]), SOS + bytes([0, 0, 0])), ("predictor Ss = 0",)),
    ("predictor-8", _patch(SOS + bytes([1, 0, 0]), SOS + bytes([8, 0, 0])), ("predictor Ss = 8",)),
    ("selector", _patch(SOS, SOS[:-1] + b"\x30"), ("component 2 selects table 3, which no DHT defines",)),
]


def _dht_mangle(counts=None, value=None):
    def mangle(k, stream, info):
        if k != 1:
            return stream
        at = stream.index(b"\xff\xc4") + 5       # the counts of table 0
        s = bytearray(stream)
        if counts is not None:
            n = sum(s[at:at + 16])
            s[at:at + 16] = counts
            assert sum(counts) == n             # (the segment's length stays what the marker says)
        if value is not None:
            s[at + 16] = value
        return bytes(s)
    return mangle


@pytest.mark.parametrize("name,mangle,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_new_refusals_name_the_segment_and_what_was_found(tmp_path, name, mangle, words):
    stored = LC.Case("r", 9, 18, 12, ncomp=2, rows_per_strip=3, fill="smooth").stored()
    p = str(tmp_path / "r.dng")
    LC.write_dng(p, stored, 12, ncomp=2, rows_per_strip=3, mangle=mangle)
    with pytest.raises(InvalidOptionError) as e:
        dng.read(p)
    assert (e.value.option, e.value.value) == ("Compression", 7)
    for w in ("lossless JPEG", "segment 1") + tuple(words):
        assert w in str(e.value), (w, str(e.value))


def test_table_and_file_structure_refusals(tmp_path):
    stored = LC.Case("r", 9, 18, 12, ncomp=2, rows_per_strip=3, fill="smooth").stored()
    p = str(tmp_path / "r.dng")

    def refused(*words, **kw):
        LC.write_dng(p, stored, 12, ncomp=2, rows_per_strip=3, **kw)
        with pytest.raises(InvalidOptionError) as e:
            dng.read(p)
        assert (e.value.option, e.value.value) == ("Compression", 7)
        for w in ("lossless JPEG",) + words:
            assert w in str(e.value), (w, str(e.value))
    # a DHT whose counts overflow the code space: three codes of one bit (the known table has 12 values: 3 + 9 keeps the length)
    refused("segment 1", "overflows the code space at length 1", tables=LC.KNOWN_TABLE, mangle=_dht_mangle(counts=[3, 9] + [0] * 14))
    refused("segment 1", "holds the category 17", tables=LC.KNOWN_TABLE, mangle=_dht_mangle(value=17))
    refused("StripByteCounts is missing", drop=(279,))
    refused("segment 2", "ends outside the", extra={279: (4, [200, 200, 100000])})
    LC.write_dng(p, stored, 12, ncomp=2, tile=(16, 16), drop=(325,))
    with pytest.raises(InvalidOptionError, match="lossless JPEG: TileByteCounts is missing"):
        dng.read(p)
    # a predictor that keeps the line above, on a segment wider than the decoder holds
    wide = np.zeros((2, _lib.LJPEG_MAX_LINE + 2), np.int64)
    LC.write_dng(p, wide, 12, ncomp=2, predictor=2)
    with pytest.raises(InvalidOptionError, match=r"lossless JPEG: segment 0: predictor Ss = 2 on a segment of 24578 columns"):
        dng.read(p)
    # deflate and lossy JPEG are refused as before
    for comp, kind in ((8, "deflate"), (34892, "lossy JPEG"), (5, "compressed samples are not read")):
        LC.write_dng(p, stored, 12, ncomp=2, extra={259: (3, [comp])})
        with pytest.raises(InvalidOptionError) as e:
            dng.read(p)
        assert (e.value.option, e.value.value) == ("Compression", comp) and kind in str(e.value)


def test_an_uncompressed_file_tagged_7_is_still_refused_by_name(tmp_path):
    c = DC.BY_NAME["12bit-5x9"]
    p = str(tmp_path / "u.dng")
    DC.write_dng(p, c.stored(), 12, extra={259: (3, [7])})
    with pytest.raises(InvalidOptionError) as e:
        dng.read(p)
    for w in ("Compression", "7", "lossless JPEG", "segment 0", "does not start with SOI"):
        assert w in str(e.value)


@pytest.mark.parametrize("name", ["12bit-5x9", "10bit-tiles-21x37-shuffled", "14bit-crop-3-5-tiles", "12bit-table-short"])
def test_an_uncompressed_case_parses_exactly_as_before(tmp_path, name):
    c = DC.BY_NAME[name]
    p = str(tmp_path / "u.dng")
    info = c.write(p)
    frame = dng.read(p)
    lay = frame.layout
    assert lay.compression == 1 and lay.segments is None and lay.counts is None
    offs = np.array(info["offsets"])
    assert lay.offsets.tolist() == (offs - offs.min()).tolist()
    rows = [lay.seg_height if lay.tiled else min(lay.seg_height, c.h - (k // lay.grid[1]) * lay.seg_height) for k in range(len(offs))]
    assert [lay.segment_bytes(k) for k in range(len(offs))] == [r * ((lay.seg_width * c.bits + 7) // 8) for r in rows]
    import unpack_restatement as UR
    assert np.array_equal(UR.unpack_layout(frame.span, lay), c.expected())
    assert [f[0] for f in lay.struct()._fields_] == [f[0] for f in _lib.RawLayoutStruct._fields_]
