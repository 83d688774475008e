"""CPU: the LinearRaw side of the DNG parser against the writer of tests/linear_cases.py -- which IFD is chosen, the layout in
samples, the quantised Linear, every new refusal with its tag's name and value, what is skipped and what remains -- the Linear
class, the restatement on values followed by hand, and that no kernel case of the table is vacuous."""
import numpy as np
import pytest

import dng_cases as DC
import linear_cases as LC
import linear_restatement as LR
import unpack_restatement as UR
from shinestacker_amd import _lib, demosaic, dng
from shinestacker_amd.errors import ImageLoadError, InvalidOptionError
from shinestacker_amd.lens import Lens


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    d = tmp_path_factory.mktemp("linear")
    out = {}
    for c in LC.FILE_CASES:
        info = c.write(str(d / (c.name + ".dng")))
        out[c.name] = (dng.read(str(d / (c.name + ".dng"))), info)
    return out


def test_linearraw_is_read(tmp_path):
    """the one that proves the feature: before it, dng.read raised ImageLoadError("no CFA IFD ...") on this file"""
    c = LC.FILES["16bit-rgb-5x17"]
    c.write(str(tmp_path / "a.dng"))
    f = dng.read(str(tmp_path / "a.dng"))
    assert f.cfa is None and isinstance(f.linear, demosaic.Linear) and f.linear.spp == 3
    assert f.shape == (5, 17) and f.dtype == np.uint16 and f.layout.spp == 3
    assert np.array_equal(UR.unpack_layout(f.span, f.layout).reshape(5, 17, 3), c.expected())


@pytest.mark.parametrize("case", LC.FILE_CASES, ids=repr)
def test_parser_returns_the_writers_layout_in_samples(case, written):
    frame, info = written[case.name]
    lay, spp = frame.layout, case.spp
    top, left, ch, cw = case.crop()
    assert lay.spp == spp and frame.cfa is None and frame.linear.spp == spp
    assert (lay.bits, lay.big_endian) == (case.bits, case.kw.get("e", "<") == ">")
    assert (lay.image_height, lay.image_width) == (case.h, case.w * spp)
    tile = case.kw.get("tile")
    assert (lay.tiled, lay.seg_height, lay.seg_width) == ((True, tile[0], tile[1] * spp) if tile else
                                                        (False, case.kw.get("rows_per_strip") or case.h, case.w * spp))
    assert (lay.crop_y, lay.crop_x, lay.height, lay.width) == (top, left * spp, ch, cw * spp)
    assert frame.shape == (ch, cw) and frame.dtype == case.dtype and lay.shift == case.shift()
    offs = np.array(info["offsets"])
    assert lay.offsets.tolist() == (offs - offs.min()).tolist()
    s = lay.struct()        # mi_raw_layout_t is unchanged: it carries the sample counts
    assert (s.image_width, s.seg_width, s.crop_x, s.width) == (lay.image_width, lay.seg_width, lay.crop_x, lay.width)
    assert not hasattr(s, "spp")
    # the restatement of raw_unpack on this layout yields the H x W x spp frame the writer stored
    got = UR.unpack_layout(frame.span, lay).reshape((ch, cw, 3) if spp == 3 else (ch, cw))
    assert got.dtype == case.dtype and np.array_equal(got, case.expected())


@pytest.mark.parametrize("case", LC.FILE_CASES, ids=repr)
def test_parser_quantises_the_levels_as_cfa_does(case, written):
    frame, _ = written[case.name]
    black, gain_q = case.linear_ints()
    assert frame.linear.black == black and frame.linear.gain_q == gain_q and frame.linear.white is None
    b, g, w, spp = frame.linear.quantised(case.dtype)
    assert (list(b), list(g), w, spp) == (black, gain_q, int(np.iinfo(case.dtype).max), case.spp)
    assert max(gain_q) < 1 << 16
    s = frame.linear.struct(case.dtype)
    assert list(s.black)[:spp] == black and list(s.gain_q)[:spp] == gain_q and (s.white, s.spp) == (w, spp)


def test_the_cases_cover_what_the_issue_names(written):
    names = set(LC.FILES)
    assert {c.spp for c in LC.FILE_CASES} == {1, 3}
    assert any(c.kw.get("sub_ifd") for c in LC.FILE_CASES) and any("active_area" in c.kw for c in LC.FILE_CASES)
    assert any("table" in c.kw for c in LC.FILE_CASES) and any(c.kw.get("tile") for c in LC.FILE_CASES)
    assert any(len(np.atleast_1d(c.kw.get("black", 0))) == 3 for c in LC.FILE_CASES)
    assert any(len(np.atleast_1d(c.kw.get("black", 0))) == 1 and "black" in c.kw for c in LC.FILE_CASES)
    # the active area of the tiled case starts inside a tile, not on a tile's edge
    c = LC.FILES["12bit-rgb-tiles-21x37-active-area"]
    assert c.crop()[0] % 16 and c.crop()[1] % 16 and c.crop()[1] // 16 == 1
    # per-sample levels really differ, and the white balance moves the gains apart
    f = written["12bit-rgb-levels-per-sample"][0]
    assert len(set(f.linear.black)) == 3 and len(set(f.linear.gain_q)) == 3
    # one sample per pixel: AsShotNeutral is not applied
    f = written["12bit-grey-levels"][0]
    assert f.linear.gains == [pytest.approx(65535 / ((4000 - 64) << 4), rel=1e-12)]
    assert "16bit-rgb-sub-ifd" in names
    f = written["16bit-rgb-sub-ifd"][0]
    assert np.allclose(f.develop.matrix, dng.colour_matrix([round(v * 10000) / 10000 for v in DC.XYZ_D65_MATRIX]), atol=1e-12)
    assert f.linear.gains == [pytest.approx(2.0), pytest.approx(1.0), pytest.approx(1.6)]


def test_a_cfa_ifd_wins_over_a_linear_one_and_neither_is_todays_error(tmp_path):
    # a file whose IFD0 is LinearRaw with NewSubFileType 1 (a preview) and nothing else: today's error, its text unchanged
    c = LC.FILES["8bit-rgb-5x17"]
    LC.write_linear(str(tmp_path / "p.dng"), c.stored(), 8, extra={254: (4, [1])})
    with pytest.raises(ImageLoadError) as ei:
        dng.read(str(tmp_path / "p.dng"))
    assert "no CFA IFD" in str(ei.value) and "32803" in str(ei.value)
    # a CFA file is read as before: linear is None
    cc = DC.BY_NAME["8bit-5x17"]
    cc.write(str(tmp_path / "c.dng"))
    f = dng.read(str(tmp_path / "c.dng"))
    assert f.linear is None and f.cfa is not None and f.layout.spp == 1 and f.shape == (f.layout.height, f.layout.width)


def _refused(tmp_path, name, value_text, **kw):
    c = LC.FILES["12bit-rgb-5x17"]
    args = dict(spp=3)
    args.update(kw)
    stored = args.pop("stored", c.stored())
    LC.write_linear(str(tmp_path / "r.dng"), stored, args.pop("bits", 12), **args)
    with pytest.raises(InvalidOptionError) as ei:
        dng.read(str(tmp_path / "r.dng"))
    assert name in str(ei.value) and value_text in str(ei.value), str(ei.value)
    return str(ei.value)


def test_every_new_refusal_names_its_tag_and_value(tmp_path):
    grey = LC.FILES["12bit-grey-5x17"].stored()
    _refused(tmp_path, "SamplesPerPixel", "2", extra={277: (3, [2])})
    _refused(tmp_path, "SamplesPerPixel", "4", extra={277: (3, [4])})
    _refused(tmp_path, "PlanarConfiguration", "2", extra={284: (3, [2])})
    _refused(tmp_path, "BitsPerSample", "(12, 12, 10)", extra={258: (3, [12, 12, 10])})
    _refused(tmp_path, "BitsPerSample", "(12, 12)", extra={258: (3, [12, 12])})
    _refused(tmp_path, "BitsPerSample", "9", stored=grey, spp=1, extra={258: (3, [9])})
    _refused(tmp_path, "BlackLevelRepeatDim", "(2, 2)", extra={50713: (3, [2, 2]), 50714: (4, [1, 2, 3, 4])})
    _refused(tmp_path, "BlackLevel", "[1, 2]", extra={50714: (4, [1, 2])})
    _refused(tmp_path, "BlackLevel", "4095", black=(0, 4095, 0))
    _refused(tmp_path, "WhiteLevel", "(4000, 4001)", extra={50717: (4, [4000, 4001])})
    _refused(tmp_path, "WhiteLevel", "70000", extra={50717: (4, [4000, 70000, 4000])})
    _refused(tmp_path, "ActiveArea", "(0, 0, 5, 18)", active_area=(0, 0, 5, 18))
    _refused(tmp_path, "Compression", "deflate", extra={259: (3, [8])})
    _refused(tmp_path, "Orientation", "9", orientation=9)


# ------------------------------------------------------------------------------------------------ skipped and remaining
def _gain_map(h, w):
    import struct
    return 9, struct.pack(">10I", 0, 0, h, w, 0, 1, 1, 1, 1, 1) + struct.pack(">4d", 1.0, 1.0, 0.0, 0.0) + struct.pack(">I", 1) + struct.pack(">f", 1.5)


def _vignette():
    import struct
    return 3, struct.pack(">7d", 0.3, 0.1, 0.0, 0.0, 0.0, 0.5, 0.5)


def test_per_site_corrections_are_skipped_with_their_reason_and_remain(tmp_path):
    import struct
    c = LC.FILES["12bit-rgb-5x17"]
    bad_list = (5, struct.pack(">3I", 0, 1, 0) + struct.pack(">2I", 1, 1))
    bad_const = (4, struct.pack(">2I", 0, 0))
    LC.write_linear(str(tmp_path / "s.dng"), c.stored(), 12, opcodes2=[_gain_map(5, 17), bad_list, bad_const],
                    opcodes3=[DC.WARP, _vignette()], orientation=6,
                    extra={50715: (10, [DC.rational(1.0)] * 17), 50716: (10, [DC.rational(1.0)] * 5), 50719: (4, [1, 1]), 50720: (4, [15, 3])})
    f = dng.read(str(tmp_path / "s.dng"))
    reason = "LinearRaw frame"
    assert sorted(f.corrections.skipped) == sorted([("BlackLevelDeltaH", reason), ("BlackLevelDeltaV", reason), ("GainMap", reason),
                                                    ("FixBadPixelsList", reason), ("FixBadPixelsConstant", reason)])
    assert f.corrections.empty and f.corrections.applies == ()
    assert f.finish.skipped == (("FixVignetteRadial", reason),) and f.finish.vignette is None
    # applied: the lens (in PIXEL coordinates), the default crop and the orientation
    assert f.lens == Lens.from_warp_rectilinear((1.0, -0.05, 0.01, 0.0, 0.0, 0.0), centre=(0.5 * 16, 0.5 * 4))
    assert f.finish.crop == (1, 1, 3, 15) and f.finish.orientation == 6 and f.finished_shape("auto") == (15, 3)
    per_site = ["BlackLevelDeltaH", "BlackLevelDeltaV", "OpcodeList2", "GainMap", "FixBadPixelsList", "FixBadPixelsConstant", "FixVignetteRadial"]
    assert sorted(f.ignored) == sorted(per_site + ["DefaultCropOrigin", "DefaultCropSize"])
    assert sorted(f.remaining("auto", "auto")) == sorted(per_site)      # every per-site correction stays in what is not applied
    assert sorted(f.remaining(None, None)) == sorted(f.ignored)
    assert dng.resolve_corrections(f, "auto") is None


def test_what_a_linear_frame_does_not_take_is_refused_by_name(tmp_path):
    c = LC.FILES["12bit-rgb-5x17"]
    c.write(str(tmp_path / "a.dng"))
    f = dng.read(str(tmp_path / "a.dng"))
    dark = np.zeros((5, 17), np.uint16)
    sc = dng.SiteCorrections(bad_sites=[3])
    vig = dng.Finish(vignette=dng.RadialGain((0.3, 0.1, 0, 0, 0), (8, 2)))
    dev = demosaic.Develop(defects=np.array([[1, 1]]))
    for kw, name in ((dict(calibration=demosaic.Calibration(dark=dark)), "calibration"), (dict(corrections=sc), "corrections"),
                     (dict(finish=vig), "finish"), (dict(develop=dev), "develop")):
        with pytest.raises(InvalidOptionError) as ei:
            dng.develop(f, **kw)
        assert name in str(ei.value) and "LinearRaw" in str(ei.value), str(ei.value)
    for kw, name in ((dict(corrections=sc), "corrections"), (dict(finish=vig), "finish")):
        with pytest.raises(InvalidOptionError) as ei:
            dng.unpack(f, **kw)
        assert name in str(ei.value) and "LinearRaw" in str(ei.value)
    lin = demosaic.Linear()
    a = np.zeros((2, 2, 3), np.uint8)
    for kw in (dict(develop=dev), dict(finish=vig)):
        with pytest.raises(InvalidOptionError):
            demosaic.develop_linear(a, lin, **kw)


# ------------------------------------------------------------------------------------------------ Linear, the restatement
def test_linear_checks_its_arguments():
    lin = demosaic.Linear(black=3, gains=1.5, spp=3)
    assert lin.black == [3, 3, 3] and lin.gain_q == [6144] * 3 and lin.white is None and lin.spp == 3
    assert demosaic.Linear(black=[1], gains=[2.0], spp=1).quantised(np.uint8) == ((1,), (8192,), 255, 1)
    assert demosaic.Linear(black=(1, 2, 3), gains=(1, 2, 3.5), white=200).quantised(np.uint8) == ((1, 2, 3), (4096, 8192, 14336), 200, 3)
    for kw, name in ((dict(spp=2), "spp"), (dict(spp=4), "spp"), (dict(black=(1, 2)), "black"), (dict(black=-1), "black"),
                     (dict(gains=16.0), "gains"), (dict(gains=(1.0, 2.0)), "gains"), (dict(gains=float("nan")), "gains"),
                     (dict(white=0), "white"), (dict(white=70000), "white"), (dict(black=1.5), "black")):
        with pytest.raises(InvalidOptionError) as ei:
            demosaic.Linear(**kw)
        assert name in str(ei.value)
    with pytest.raises(InvalidOptionError):
        demosaic.Linear(white=300).quantised(np.uint8)
    with pytest.raises(InvalidOptionError):
        demosaic.check_samples(np.zeros((2, 2), np.uint8), demosaic.Linear(spp=3))
    with pytest.raises(InvalidOptionError):
        demosaic.check_samples(np.zeros((2, 2, 3), np.uint8), demosaic.Linear(spp=1))


def test_restatement_by_hand():
    # one pixel, uint8: R = 10, G = 200, B = 255 with black (12, 8, 0), gains (2, 1, 0.5), white 250
    px = np.array([[[10, 200, 255]]], np.uint8)
    out = LR.linear_develop(px, (12, 8, 0), (8192, 4096, 2048), 250)
    #   R: below black -> 0;  G: (192 * 4096 + 2048) >> 12 = 192;  B: (255 * 2048 + 2048) >> 12 = 128
    assert out.tolist() == [[[128, 192, 0]]]        # BGR
    out = LR.linear_develop(np.array([[[255, 255, 255]]], np.uint8), (0, 0, 0), (8192, 4096, 4096), 250)
    assert out.tolist() == [[[250, 250, 250]]]      # clamped at white
    # one sample per pixel: b = g = r
    assert LR.linear_develop(np.array([[7, 9]], np.uint16), (1,), (4096 * 3,)).tolist() == [[[18, 18, 18], [24, 24, 24]]]
    # the matrix sees (r, g, b) and the tone table the result
    m = (0, 4096, 0, 0, 0, 4096, 4096, 0, 0)        # R' = G, G' = B, B' = R
    out = LR.linear_develop(np.array([[[1, 2, 3]]], np.uint8), matrix_q=m, tone=(255 - np.arange(256)).astype(np.uint8))
    assert out.tolist() == [[[255 - 1, 255 - 3, 255 - 2]]]


def test_no_kernel_case_is_vacuous():
    """each shape of the GPU test hits the path it is there for, by the constants the kernel exports"""
    for dt in (np.uint8, np.uint16):
        span = _lib.linear_span(dt)         # (the library's own figure: 256 threads x 4 groups of 4 / itemsize pixels)
        assert span == {1: 4096, 2: 2048}[np.dtype(dt).itemsize]
        shapes = LC.kernel_shapes(dt, span)
        P = {n: LC.kernel_paths(h, w, dt, span) for n, (h, w) in shapes.items()}
        assert P["1x1"] == {"ragged"} and "wide" in P["1xN"] and "wide" in P["Nx1"]
        assert "second workgroup" not in P["span"] and "second workgroup" not in P["span-1"] and "ragged" in P["span-1"]
        assert P["span+1"] == {"wide", "ragged", "second workgroup"}
        assert "second workgroup" in P["two-rows-past-two-spans"] and shapes["two-rows-past-two-spans"][0] * 64 == 2 * span + 128
        # widths 1 to 9 at three rows: rows that start off a 4-byte boundary, and both a ragged and an even end
        assert {n for n in shapes if n.startswith("3x")} == {f"3x{w}" for w in range(1, 10)}
        assert any("ragged" in P[f"3x{w}"] for w in range(1, 10)) and any("ragged" not in P[f"3x{w}"] for w in range(1, 10))
        assert LC.kernel_paths(3, 5, dt, span, dst_misaligned=True) == {"unaligned"}
    # the special values are really among the samples
    a = LC.samples_for(3, 5, 3, np.uint16, (100, 90, 80), 60000).reshape(-1)
    assert a[0] == 79 and a[2] == 60000 and a[3] == 65535


def test_library_states_the_same_span(hiplib):
    lib = hiplib.load()
    assert lib.mi_linear_span(hiplib.MI_U8) == hiplib.linear_span(np.uint8) == 4096
    assert lib.mi_linear_span(hiplib.MI_U16) == hiplib.linear_span(np.uint16) == 2048
    assert lib.mi_linear_span(hiplib.MI_F32) == 0


# ------------------------------------------------------------------------------------------------ three-component lossless JPEG
@pytest.fixture(scope="module")
def ljpeg3_written(tmp_path_factory):
    d = tmp_path_factory.mktemp("ljpeg3")
    out = {}
    for c in LC.LJPEG3_CASES + [LC.LJPEG3_SHORT[0]]:
        info = c.write(str(d / (c.name + ".dng")))
        out[c.name] = (dng.read(str(d / (c.name + ".dng"))), info)
    return out


@pytest.mark.parametrize("case", LC.LJPEG3_CASES, ids=repr)
def test_parser_fills_three_component_descriptors(case, ljpeg3_written):
    import ljpeg_restatement as JR
    frame, info = ljpeg3_written[case.name]
    lay = frame.layout
    assert lay.compression == 7 and lay.spp == 3 and lay.segments.dtype == _lib.LJPEG_SEG3_DTYPE
    tile = case.tile_px
    assert (lay.tiled, lay.seg_height, lay.seg_width) == ((True, tile[0], 3 * tile[1]) if tile else
                                                        (False, case.kw.get("rows_per_strip") or case.h, 3 * case.wpx))
    lo = min(info["offsets"])
    for k, (off, stream, i) in enumerate(zip(info["offsets"], info["streams"], info["infos"])):
        s = lay.segments[k]
        assert (s["ncomp"], s["predictor"], s["precision"]) == (3, case.predictor, case.precision)
        assert s["x"] * 3 == lay.seg_width and s["y"] == lay.segment_rows(k)
        assert (s["scan_off"], s["scan_bytes"]) == (off - lo + i["scan_off"], len(stream) - i["scan_off"])
        for c, (counts, values) in enumerate(i["tables"]):
            assert s["counts"][c].tolist() == counts and s["values"][c][:len(values)].tolist() == values
    # the restatement places the three components along the row: H x 3W samples are the H x W x 3 frame
    got, status = LR.unpack_three(frame.span, lay)
    assert got.shape == frame.shape + (3,) and not status.any() and np.array_equal(got, case.expected_px())
    assert np.array_equal(got.reshape(lay.height, lay.width), JR.unpack_layout(frame.span, lay)[0])


def test_no_ljpeg3_case_is_vacuous(ljpeg3_written):
    B = _lib.ljpeg3_batch()     # (the library's own figure)
    assert B == 192 and LC.BATCH3_PX * 3 == B
    widths = {c.name: 3 * c.wpx for c in LC.LJPEG3_CASES}
    assert widths["12bit-one-pixel"] == 3 and widths["12bit-3x63-one-batch-minus-one"] == B - 3 and widths["12bit-3x64-one-batch"] == B
    assert widths["12bit-3x65-one-batch-plus-one"] == B + 3 and widths["14bit-3x129-two-batches-plus-one"] == 2 * B + 3
    assert {c.predictor for c in LC.LJPEG3_CASES if c.h > 1 and 3 * c.wpx > B} >= set(range(1, 8))     # carry and every predictor
    c = LC.LJPEG3["16bit-file-12bit-precision"]
    assert c.precision < c.bits
    c = LC.LJPEG3["14bit-strips-of-3-short-last"]
    assert c.h % c.kw["rows_per_strip"] and ljpeg3_written[c.name][0].layout.segment_rows(2) == 1
    c = LC.LJPEG3["12bit-tiles-21x37-shuffled-active-area"]
    assert c.crop_px()[0] % 16 and c.crop_px()[1] % 16 and sorted(c.kw["order"]) != list(c.kw["order"])
    # different tables per component and per tile
    segs = ljpeg3_written[c.name][0].layout.segments
    assert len({bytes(segs[k]["counts"][0]) for k in range(len(segs))}) > 1
    assert any(bytes(s["counts"][0]) != bytes(s["counts"][1]) or bytes(s["counts"][1]) != bytes(s["counts"][2]) for s in segs)
    # the all-stuffed case: every data byte pair is FF 00; a long stream outgrows the ring
    info = ljpeg3_written["16bit-flip-32768-all-stuffed"][1]
    assert info["infos"][0]["stuffed"] * 2 >= info["infos"][0]["data_bytes"] - 2
    assert ljpeg3_written["16bit-40x70-random-long-stream"][1]["infos"][0]["data_bytes"] > 4096
    assert ljpeg3_written["16bit-long-codes-p5"][1]["infos"][0]["longest"] > 10
    # the cut stream: the restatement flags exactly its segment
    import ljpeg_restatement as JR
    case, seg, flag = LC.LJPEG3_SHORT
    frame = ljpeg3_written[case.name][0]
    assert JR.unpack_layout(frame.span, frame.layout)[1].tolist() == [flag if k == seg else 0 for k in range(3)]


def test_other_component_counts_are_refused_by_name(tmp_path):
    import ljpeg_cases as LJ
    stored = np.arange(4 * 6, dtype=np.int64).reshape(4, 6) + 100
    tags = {262: (3, [LC.LINEAR]), 277: (3, [3]), 258: (3, [12, 12, 12]), 256: (4, [2])}
    for nf in (1, 2):       # a three-sample frame whose streams hold 1 or 2 components
        LJ.write_dng(str(tmp_path / "n.dng"), stored, 12, ncomp=nf, extra=tags, drop=LC.CFA_TAGS)
        with pytest.raises(InvalidOptionError) as ei:
            dng.read(str(tmp_path / "n.dng"))
        assert "Compression" in str(ei.value) and f"Nf = {nf} components" in str(ei.value) and "Nf = 3" in str(ei.value)
    # one sample per pixel: Nf 1 and 2 go through the existing two-table path, Nf = 3 is refused there in today's words
    grey = {262: (3, [LC.LINEAR]), 277: (3, [1]), 258: (3, [12])}
    for nf in (1, 2):
        LJ.write_dng(str(tmp_path / "g.dng"), stored, 12, ncomp=nf, extra=grey, drop=LC.CFA_TAGS)
        f = dng.read(str(tmp_path / "g.dng"))
        assert f.linear.spp == 1 and f.layout.segments.dtype == _lib.LJPEG_SEG_DTYPE and f.layout.segments["ncomp"][0] == nf
    LJ.write_dng(str(tmp_path / "g3.dng"), stored, 12, ncomp=3, extra=grey, drop=LC.CFA_TAGS)
    with pytest.raises(InvalidOptionError) as ei:
        dng.read(str(tmp_path / "g3.dng"))
    assert "Nf = 3 components (1 or 2 are read)" in str(ei.value)
