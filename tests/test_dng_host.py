"""CPU: the DNG parser against the independent writer of tests/dng_cases.py -- geometry, Cfa, colour matrix, lens and `ignored` of
every case; the colour-matrix construction by hand; every refusal with its tag's name; the restatement inverts the writer's
packing; no case of the table is vacuous."""
import numpy as np
import pytest

import dng_cases as DC
import unpack_restatement as R
from shinestacker_amd import FocusStack, CombinedActions, PyramidStack, dng
from shinestacker_amd.errors import ImageLoadError, InvalidOptionError
from shinestacker_amd.lens import Lens, LensCorrection


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """{case name: (DngFrame, what the writer reported)} of the whole table, written and parsed once"""
    d = tmp_path_factory.mktemp("dng")
    out = {}
    for c in DC.CASES:
        info = c.write(str(d / (c.name + ".dng")))
        out[c.name] = (dng.read(str(d / (c.name + ".dng"))), info)
    return out


@pytest.mark.parametrize("case", DC.CASES, ids=repr)
def test_parser_returns_the_writers_geometry(case, written):
    frame, info = written[case.name]
    lay = frame.layout
    tiled, seg_h, seg_w = case.segments()
    top, left, ch, cw = case.crop()
    assert (lay.bits, lay.big_endian) == (case.bits, case.kw.get("e", "<") == ">")
    assert (lay.image_height, lay.image_width) == (case.h, case.w)
    assert (lay.tiled, lay.seg_height, lay.seg_width) == (tiled, seg_h, seg_w)
    assert (lay.crop_y, lay.crop_x, lay.height, lay.width) == (top, left, ch, cw)
    assert frame.shape == (ch, cw) and frame.dtype == lay.dtype == case.dtype
    assert lay.shift == case.shift()
    table = case.kw.get("table")
    assert (lay.table is None) == (table is None) and (table is None or lay.table.tolist() == list(table))
    # the span: from the lowest segment to the end of the highest, offsets rebased to it, the file's own bytes
    offs = np.array(info["offsets"])
    sizes = np.array([lay.segment_bytes(k) for k in range(len(offs))])
    assert lay.offsets.dtype == np.uint32 and lay.offsets.tolist() == (offs - offs.min()).tolist()
    assert frame.span.dtype == np.uint8 and frame.span.nbytes == (offs + sizes).max() - offs.min()
    with open(frame.path, "rb") as fh:
        data = fh.read()
    assert bytes(frame.span) == data[offs.min():(offs + sizes).max()]
    assert not frame.span.flags.writeable
    s = lay.struct()
    assert (s.bits, s.tiled, s.seg_height, s.seg_width, s.crop_y, s.crop_x, s.height, s.width, s.shift, s.table_len) == \
        (case.bits, int(tiled), seg_h, seg_w, top, left, ch, cw, case.shift(), 0 if table is None else len(table))


@pytest.mark.parametrize("case", DC.CASES, ids=repr)
def test_restatement_inverts_the_writers_packing(case, written):
    frame, _ = written[case.name]
    got = R.unpack_layout(frame.span, frame.layout)
    assert got.dtype == case.dtype and np.array_equal(got, case.expected())


@pytest.mark.parametrize("case", DC.CASES, ids=repr)
def test_parser_returns_the_writers_cfa(case, written):
    frame, _ = written[case.name]
    top, left, _, _ = case.crop()
    cell = case.kw.get("pattern", "RGGB")
    want = "".join(cell[2 * ((py + top) & 1) + ((px + left) & 1)] for py in range(2) for px in range(2))
    assert frame.cfa.pattern == want
    shift, white = case.shift(), case.white()
    maxv = int(np.iinfo(case.dtype).max)
    black = [int(np.floor(b + 0.5)) for b in case.kw.get("black", (0,))]
    black = black * 4 if len(black) == 1 else black
    assert frame.cfa.black == [b << shift for b in black] and frame.cfa.white is None
    n = case.kw.get("neutral")
    for pos in range(4):
        wb = 1.0 if n is None else (round(n[1] * 10000) / 10000) / (round(n["RGB".index(want[pos])] * 10000) / 10000)
        assert frame.cfa.gains[pos] == pytest.approx(wb * maxv / ((white - black[pos]) << shift), rel=1e-12)
    assert frame.orientation == case.kw.get("orientation", 1)


def test_colour_matrix_by_hand():
    """cam_from_srgb = ColorMatrix @ XYZ_from_sRGB, rows normalised, inverted -- checked on a matrix whose numbers can be
    followed by hand.  ColorMatrix = XYZ_from_sRGB^-1 with its rows scaled by (2, 1, 4): cam_from_srgb is then diag(2, 1, 4),
    every row divided by its sum is the identity, and M is the identity: a camera that sees scaled linear sRGB needs no matrix."""
    cm = np.diag([2.0, 1.0, 4.0]) @ np.linalg.inv(dng.XYZ_FROM_SRGB)
    assert np.allclose(dng.colour_matrix(cm.reshape(9)), np.eye(3), atol=1e-12)
    # and a second one: camera = a fixed mix of sRGB.  cam_from_srgb = A (rows sum to 2, 1, 1) -> normalised rows -> M = inverse
    A = np.array([[1.5, 0.5, 0.0], [0.25, 0.5, 0.25], [0.0, 0.2, 0.8]])
    M = dng.colour_matrix((A @ np.linalg.inv(dng.XYZ_FROM_SRGB)).reshape(9))
    An = np.array([[0.75, 0.25, 0.0], [0.25, 0.5, 0.25], [0.0, 0.2, 0.8]])
    # the inverse of An by cofactors: det = 0.75 (0.4 - 0.05) - 0.25 (0.2 - 0) = 0.2125
    want = np.array([[0.35, -0.2, 0.0625], [-0.2, 0.6, -0.1875], [0.05, -0.15, 0.3125]]) / 0.2125
    assert np.allclose(An @ want, np.eye(3), atol=1e-15) and np.allclose(M, want, atol=1e-12)
    assert np.allclose(M.sum(axis=1), 1.0)          # white stays white
    assert dng.XYZ_FROM_SRGB.tolist() == [[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750],
                                          [0.0193339, 0.1191920, 0.9503041]]


def test_parser_returns_the_writers_develop_lens_and_ignored(written):
    def matrix(vals):
        return dng.colour_matrix([round(v * 10000) / 10000 for v in vals])
    for c in DC.CASES:      # no colour matrix, no opcode: nothing made up
        if not c.kw.get("matrices"):
            assert written[c.name][0].develop is None, c.name
        if not c.kw.get("opcodes3"):
            assert written[c.name][0].lens is None, c.name
    # ColorMatrix2 is the D65 one; the raw IFD is a SubIFD and the colour tags sit in IFD0
    f = written["12bit-sub-ifd-colour"][0]
    assert np.allclose(f.develop.matrix, matrix(DC.XYZ_D65_MATRIX), atol=1e-12)
    assert np.array_equal(f.develop.tone, dng.srgb_tone(np.uint16))
    assert f.lens == Lens.from_warp_rectilinear((1.0, -0.05, 0.01, 0.0, 0.0, 0.0), centre=(0.5 * 9, 0.5 * 5))
    assert f.ignored == () and f.orientation == 6
    # ColorMatrix1 is the D65 one: it wins over ColorMatrix2
    f = written["14bit-colour-rational-black"][0]
    assert np.allclose(f.develop.matrix, matrix(DC.XYZ_D65_MATRIX), atol=1e-12)
    assert f.lens == Lens(((0.99, 0, 0, 0), (1, 0, 0, 0), (1.01, 0, 0, 0)), centre=(0.4 * 9, 0.6 * 5))    # the opcode is R, G, B
    assert sorted(f.ignored) == sorted(["BlackLevelDeltaH", "AnalogBalance", "DefaultCropOrigin", "DefaultCropSize", "OpcodeList2",
                                        "GainMap", "GainMap"])
    assert f.cfa.black == [1024 << 2] * 4           # RATIONAL 1023.6, rounded
    # no D65 matrix: ColorMatrix2; tangential terms: the opcode is reported, not applied
    f = written["12bit-colour-no-d65"][0]
    assert np.allclose(f.develop.matrix, matrix(DC.XYZ_D65_MATRIX), atol=1e-12)
    assert f.lens is None and f.ignored == ("WarpRectilinear (tangential terms)",)
    f = written["12bit-colour-matrix1-only"][0]
    assert np.allclose(f.develop.matrix, matrix(DC.OTHER_MATRIX), atol=1e-12)


REFUSALS = [
    ("Compression", dict(extra={259: (3, [7])}), InvalidOptionError, ("Compression", "7", "lossless JPEG")),
    ("Compression", dict(extra={259: (3, [8])}), InvalidOptionError, ("Compression", "8", "deflate")),
    ("Compression", dict(extra={259: (3, [34892])}), InvalidOptionError, ("Compression", "34892", "lossy JPEG")),
    ("Compression", dict(extra={259: (3, [5])}), InvalidOptionError, ("Compression", "5")),
    ("SamplesPerPixel", dict(extra={277: (3, [3])}), InvalidOptionError, ("SamplesPerPixel", "3")),
    ("CFARepeatPatternDim", dict(extra={33421: (3, [6, 6])}), InvalidOptionError, ("CFARepeatPatternDim", "(6, 6)")),
    ("CFALayout", dict(extra={50711: (3, [2])}), InvalidOptionError, ("CFALayout", "2")),
    ("CFAPlaneColor", dict(extra={50710: (1, [0, 1, 2, 3])}), InvalidOptionError, ("CFAPlaneColor",)),
    ("CFAPattern", dict(extra={33422: (1, [0, 0, 1, 2])}), InvalidOptionError, ("CFAPattern", "(0, 0, 1, 2)")),
    ("BitsPerSample", dict(extra={258: (3, [11])}), InvalidOptionError, ("BitsPerSample", "11")),
    ("BitsPerSample", dict(extra={258: (3, [32])}), InvalidOptionError, ("BitsPerSample", "32")),
    ("ActiveArea", dict(active_area=(0, 0, 7, 8)), InvalidOptionError, ("ActiveArea", "(0, 0, 7, 8)")),
    ("WhiteLevel", dict(white=70000), InvalidOptionError, ("WhiteLevel", "70000")),
    ("BlackLevel", dict(black=(5000,)), InvalidOptionError, ("BlackLevel", "5000")),
    ("BlackLevelRepeatDim", dict(extra={50713: (3, [1, 2]), 50714: (3, [1, 2])}), InvalidOptionError, ("BlackLevelRepeatDim", "(1, 2)")),
    ("StripByteCounts", dict(extra={279: (4, [71])}), ImageLoadError, ("truncated segment", "StripByteCounts[0] = 71", "72")),
    ("StripOffsets", dict(extra={273: (4, [100000])}), ImageLoadError, ("truncated segment", "StripOffsets[0] = 100000")),
    ("StripOffsets", dict(extra={273: (4, [8, 9])}), InvalidOptionError, ("StripOffsets", "2")),
    ("no CFA IFD", dict(extra={262: (3, [2])}), ImageLoadError, ("no CFA IFD", "32803")),
    ("no CFA IFD", dict(extra={254: (4, [1])}), ImageLoadError, ("no CFA IFD",)),
]


@pytest.mark.parametrize("what,kw,exc,words", REFUSALS, ids=[f"{r[0]}-{i}" for i, r in enumerate(REFUSALS)])
def test_refusals_name_the_tag_and_its_value(tmp_path, what, kw, exc, words):
    stored = np.arange(48).reshape(6, 8)       # 12 bits: 12 bytes a row, 72 bytes
    DC.write_dng(str(tmp_path / "r.dng"), stored, 12, **kw)
    with pytest.raises(exc) as e:
        dng.read(str(tmp_path / "r.dng"))
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_more_refusals(tmp_path):
    stored = np.arange(48).reshape(6, 8)
    p = str(tmp_path / "t.dng")
    DC.write_truncated(p, stored, 12, cut=1)                         # the file ends a byte early
    with pytest.raises(ImageLoadError, match=r"truncated segment: StripOffsets\[0\]"):
        dng.read(p)
    DC.write_truncated(p, stored, 12, cut=3, byte_counts=True)       # the file is whole, StripByteCounts says less
    with pytest.raises(ImageLoadError, match=r"truncated segment: StripByteCounts\[0\] = 69"):
        dng.read(p)
    DC.write_dng(p, stored, 8, table=list(range(256)))
    with pytest.raises(InvalidOptionError, match="LinearizationTable"):
        dng.read(p)
    DC.write_dng(p, stored, 12, tile=(16, 16), extra={325: (4, [300])})
    with pytest.raises(ImageLoadError, match=r"truncated segment: TileByteCounts\[0\] = 300"):
        dng.read(p)
    with open(p, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + b"\0" * 32)
    with pytest.raises(ImageLoadError, match="not a TIFF"):
        dng.read(p)
    with pytest.raises(RuntimeError, match="File does not exist"):
        dng.read(str(tmp_path / "missing.dng"))


def test_no_case_is_vacuous(written):
    """each edge the table claims is hit: predicted from the geometry, as tests/lens_cases.py does for its loads"""
    seen = {c.name: DC.paths(c, written[c.name][0].layout.offsets, written[c.name][0].span.nbytes) for c in DC.CASES}
    every = set().union(*seen.values())
    assert every == set(DC.PATHS), set(DC.PATHS) - every
    for bits in (10, 12, 14):
        assert seen[f"{bits}bit-5x2"] == {"partial"} and seen[f"{bits}bit-2x3"] == {"partial"} and seen[f"{bits}bit-5x7"] == {"partial"}
        assert "whole" in seen[f"{bits}bit-2x8"] and "partial" not in seen[f"{bits}bit-2x8"]        # exactly one window a row
        assert {"whole", "partial"} <= seen[f"{bits}bit-5x9"] and {"whole", "partial"} <= seen[f"{bits}bit-2x17"]   # the tail
        assert {"whole", "partial"} <= seen[f"{bits}bit-5x130"]
    assert (3 * 12) % 8 == 4 and written["12bit-2x3"][0].layout.row_bytes == 5           # half a byte of padding a row
    # a first segment at an odd file offset: windows off the dword boundary; and off the byte boundary under an odd crop
    for name in ("12bit-odd-start", "16bit-odd-start-le", "10bit-strips-of-1-shuffled-gaps-odd-start", "8bit-5x47-odd-start"):
        assert min(written[name][1]["offsets"]) % 2 == 1, name
    assert "unaligned" in seen["10bit-strips-of-1-shuffled-gaps-odd-start"]
    assert all("bit offset" in seen[f"12bit-crop-{y}-5-strips"] for y in (2, 3))
    assert {"span end"} <= seen["12bit-2x8"] | seen["12bit-odd-start"]
    # edge tiles, and windows across a tile's edge
    for name in ("12bit-tiles-21x37", "10bit-tiles-21x37-shuffled", "14bit-tiles-21x37", "16bit-tiles-21x37-be", "8bit-tiles-21x37"):
        lay = written[name][0].layout
        assert lay.grid == (2, 3) and lay.image_height % lay.seg_height and lay.image_width % lay.seg_width, name
        assert "tile-cross" in seen[name] or lay.bits == 8 and "partial" in seen[name], name
    assert "fifth dword" in seen["14bit-tiles-21x37"] and "fifth dword" in seen["16bit-tiles-21x37-be"]
    # shuffled segments with gaps: the offsets are not ascending and the span holds more than the segments
    for name in ("14bit-strips-of-3-shuffled-gaps", "10bit-strips-of-1-shuffled-gaps-odd-start", "10bit-tiles-21x37-shuffled"):
        lay, span = written[name][0].layout, written[name][0].span
        assert lay.offsets.tolist() != sorted(lay.offsets.tolist()), name
        assert span.nbytes > sum(lay.segment_bytes(k) for k in range(len(lay.offsets))), name
    # every parity of crop origin, and the four patterns that come of it
    for fam, n in (("12bit-crop-%d-%d-strips", 4), ("14bit-crop-%d-%d-tiles", 4)):
        pats = {written[fam % (y, x)][0].cfa.pattern for y in (2, 3) for x in (4, 5)}
        assert len(pats) == n
    # the table's clamp: samples beyond its last entry exist inside the crop
    for name in ("12bit-table-short", "14bit-table-short-white-4095"):
        c = DC.BY_NAME[name]
        assert (c.stored() >= len(c.kw["table"])).any() and (c.stored() < len(c.kw["table"])).any(), name
    assert {DC.BY_NAME[n].shift() for n in ("16bit-shift-0", "16bit-white-16383-shift-2", "12bit-shift-4")} == {0, 2, 4}
    assert DC.BY_NAME["14bit-white-4000-shift-4"].shift() == 4 and DC.BY_NAME["8bit-white-63-shift-2"].shift() == 2
    for name in ("12bit-ones", "10bit-ones", "14bit-ones-tiles", "16bit-ones-be"):
        c = DC.BY_NAME[name]
        assert (c.stored() == (1 << c.bits) - 1).all(), name
    assert not DC.BY_NAME["12bit-zeros"].stored().any() and not DC.BY_NAME["14bit-zeros"].stored().any()
    assert max(max(c.h, c.w) for c in DC.CASES if "530" not in c.name) <= 300


def test_options_are_checked_on_the_host(tmp_path):
    """raw= is opt-in and checked where it is given; nothing here needs a device"""
    assert dng.EXTENSIONS == frozenset(["dng"])
    from shinestacker_amd import constants
    assert "dng" not in constants.EXTENSIONS
    with pytest.raises(InvalidOptionError):
        dng.Raw(develop="srgb")
    with pytest.raises(InvalidOptionError):
        dng.Raw(lens="barrel")
    with pytest.raises(InvalidOptionError):
        PyramidStack(raw="auto")
    with pytest.raises(InvalidOptionError):
        FocusStack("s", PyramidStack(), raw=True)
    raw = dng.Raw()
    assert raw.develop == "auto" and raw.lens == "auto" and raw.calibration is None
    with pytest.raises(InvalidOptionError, match="corrected twice"):
        CombinedActions("a", [LensCorrection(Lens.distortion(-0.1))], raw=raw)
    CombinedActions("a", [LensCorrection(Lens.distortion(-0.1))], raw=dng.Raw(lens=None))
    CombinedActions("a", [LensCorrection(Lens.distortion(-0.1))])
    # the folder scan and the output names
    for n in ("a.dng", "b.DNG", "c.tif", "d.txt"):
        (tmp_path / n).write_bytes(b"")
    fs = FocusStack("s", PyramidStack(), raw=raw, input_path=str(tmp_path))
    fs.input_full_path = str(tmp_path)
    assert fs.folder_filelist() == ["a.dng", "b.DNG", "c.tif"]
    assert [fs.output_name(n) for n in ("a.dng", "b.DNG", "c.tif", "x.y.dng")] == ["a.tif", "b.tif", "c.tif", "x.y.tif"]
    assert fs.stack_algo.raw is raw
    plain = FocusStack("s", PyramidStack(), input_path=str(tmp_path))
    plain.input_full_path = str(tmp_path)
    assert plain.folder_filelist() == ["c.tif"] and plain.output_name("a.dng") == "a.dng" and plain.stack_algo.raw is None
