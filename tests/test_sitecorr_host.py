"""CPU: the site corrections' host side -- no case of tests/sitecorr_cases.py is vacuous; `quantised` by hand on a 2-node ramp;
the parser against files written with dng_cases.write_dng(opcodes2=..., extra=...); every skip reason; `remaining`."""
import numpy as np
import pytest

import dng_cases as DC
import sitecorr_cases as SC
import sitecorr_restatement as RS
from shinestacker_amd import dng
from shinestacker_amd.errors import InvalidOptionError


# ------------------------------------------------------------------------------------------------ the table is not vacuous
def test_every_predictor_path_is_taken_with_and_without_column_deltas():
    for has_dh in (False, True):
        for dt in SC.DTYPES:
            seen = set()
            for c in SC.CASES:
                if c.dtype == dt and c.deltas == has_dh:
                    seen |= SC.paths(c.h, c.w, c.dtype, has_dh)
            assert seen == {"whole", "site"}, (has_dh, dt)


def test_a_case_needs_two_workgroups_along_a_row():
    for dt in SC.DTYPES:
        assert max(SC.workgroups_along_row(c.w, c.dtype) for c in SC.CASES if c.dtype == dt) == 2
        assert all(SC.workgroups_along_row(w, dt) == 1 for _, w in SC._frames(dt))


@pytest.mark.parametrize("case", [c for c in SC.CASES if c.gains is not None], ids=repr)
def test_every_node_of_every_grid_is_read(case):
    for mask in case.nodes_read():
        assert mask.all(), f"{(~mask).sum()} of {mask.size} nodes are never read"


def test_the_named_map_shapes_and_values_are_in_the_table():
    shapes = {m.nodes.shape for c in SC.CASES if c.gains is not None
              for m in ((c.gains,) if isinstance(c.gains, dng.GainMap) else c.gains) if m is not None}
    assert {(1, 1), (1, 4), (4, 1), (2, 2), (3, 5), (9, 11), (257, 257)} <= shapes
    for dt in SC.DTYPES:
        q = SC.BY_NAME[f"{dt.name}-nodes-0-and-65535"].tables()
        assert q.gains[0][0].min() == 0 and q.gains[0][0].max() == 65535
        c = SC.BY_NAME[f"{dt.name}-four-maps-four-geometries"]
        assert len({m.nodes.shape for m in c.gains}) == 4 and len({id(g[0]) for g in c.tables().gains}) == 4
        one = SC.BY_NAME[f"{dt.name}-one-position-mapped"].tables()
        assert [g is None for g in one.gains] == [True, True, False, True]
        q = SC.BY_NAME[f"{dt.name}-outside-the-grid-on-four-sides"].tables().gains[0]
        ra, ca = q[1], q[2]
        # clamped below the first node (node 0, weight 0) and at the last (the last node, weight 0), rows and columns
        for ax, n in ((ra, q[0].shape[0]), (ca, q[0].shape[1])):
            assert (ax["node"][0], ax["weight"][0]) == (0, 0) and (ax["node"][-1], ax["weight"][-1]) == (n - 1, 0)
            assert ax["weight"].max() > 0


@pytest.mark.parametrize("case", [c for c in SC.CASES if c.deltas], ids=repr)
def test_both_ends_of_both_delta_tables_matter(case):
    q = case.tables()
    assert q.dh.dtype == q.dv.dtype == np.int16 and (len(q.dh), len(q.dv)) == (case.w, case.h)
    assert q.dh[0] < 0 < q.dh[-1] and q.dv[-1] < 0 < q.dv[0]
    # a changed end changes its corner site
    for name, at, site in (("dh", 0, (0, 0)), ("dh", -1, (0, case.w - 1)), ("dv", 0, (0, 0)), ("dv", -1, (case.h - 1, 0))):
        t = {"dh": q.dh.copy(), "dv": q.dv.copy()}
        t[name][at] = 0
        other = RS.site_correct(case.mosaic(), case.black, t["dh"], t["dv"], q.gains)
        assert other[site] != case.expected()[site], (name, at)


@pytest.mark.parametrize("case", [c for c in SC.CASES if c.gains is not None], ids=repr)
def test_at_least_half_the_sites_change_under_gains(case):
    assert (case.expected() != case.mosaic()).mean() >= 0.5


@pytest.mark.parametrize("case", SC.CASES, ids=repr)
def test_at_most_a_quarter_of_the_sites_clamp(case):
    clamped = (case.expected() == case.maxv).mean()
    if case.name in SC.SATURATING:
        assert clamped > 0.5
    else:
        assert clamped <= 0.25


def test_bad_cases_hold_sites_with_none_one_and_four_valid_neighbours():
    counts = set()
    for b in SC.BAD_CASES:
        counts |= set(b.valid_neighbours().values())
    assert {0, 1, 4} <= counts
    rect = next(b for b in SC.BAD_CASES if "rectangle" in b.name)
    assert len(rect.sites()) == 9 and min(rect.valid_neighbours().values()) < 4
    # the one-phase case: the constant lies on every position, the mask names one
    ys, xs = zip(*SC.ONE_PHASE.sites_yx)
    assert {2 * (y & 1) + (x & 1) for y, x in zip(ys, xs)} == {0, 1, 2, 3} and SC.ONE_PHASE.mask == 4
    for dt in SC.DTYPES:
        a = SC.ONE_PHASE.mosaic(dt, True)
        out = RS.repair_const(a, SC.ONE_PHASE.constant(dt), SC.ONE_PHASE.mask)
        changed = np.argwhere(out != a)
        assert len(changed) and all((y & 1, x & 1) == (1, 0) for y, x in changed)
        assert (out == SC.ONE_PHASE.constant(dt)).sum() == len(SC.ONE_PHASE.sites_yx) - len(changed)


@pytest.mark.parametrize("bad", SC.BAD_CASES, ids=repr)
def test_repair_by_list_and_by_constant_agree(bad):
    for dt in SC.DTYPES:
        by_list = RS.repair_list(bad.mosaic(dt, True), bad.sites())
        by_const = RS.repair_const(bad.mosaic(dt, True), bad.constant(dt), 15)
        assert np.array_equal(by_list, by_const)
        nv = bad.valid_neighbours()
        for (y, x), k in nv.items():
            assert (by_list[y, x] == bad.constant(dt)) == (k == 0)


# ------------------------------------------------------------------------------------------------ quantised, by hand
def test_quantised_on_a_two_node_ramp_in_closed_form():
    """nodes (1, 2) along a row, origin 0, spacing 1: t = (x + 0.5) / W, node 0, weight b = round(256 t), and the gain is
    ((256 - b) 4096 + b 8192) 256 + 32768 >> 16 = 4096 + 16 b"""
    w, h = 10, 4
    sc = dng.SiteCorrections(gains=dng.GainMap([[1.0, 2.0]], spacing=(0.0, 1.0), origin=(0.0, 0.0)))
    q = sc.quantised((h, w), np.uint16)
    assert all(g is q.gains[0] for g in q.gains)
    nodes, ra, ca = q.gains[0]
    assert nodes.dtype == np.uint16 and nodes.tolist() == [[4096, 8192]]
    assert ra["node"].tolist() == [0] * h and ra["weight"].tolist() == [0] * h
    b = [int(np.floor(256 * (x + 0.5) / w + 0.5)) for x in range(w)]
    assert ca["node"].tolist() == [0] * w and ca["weight"].tolist() == b
    g = RS.gain_plane((h, w), q.gains)
    assert g.tolist() == [[4096 + 16 * v for v in b]] * h
    # round-half-up of node * 4096, clipped at 65535; deltas as int16
    assert dng.GainMap([[15.99999, 0.00012, 0.000123]]).nodes_q().tolist() == [[65535, 0, 1]]
    q = dng.SiteCorrections(black_h=[1, -2, 3], black_v=[-4, 5]).quantised((2, 3), np.uint8)
    assert q.dh.tolist() == [1, -2, 3] and q.dv.tolist() == [-4, 5] and q.flags == 3


def test_relative_is_the_pixel_centre():
    assert dng.relative(0, 4) == 0.125 and dng.relative(3, 4) == 0.875


def test_constructor_refuses_what_the_kernel_cannot_take():
    for kw in (dict(black_h=[0.5, 1.0]), dict(black_h=[40000, 0]), dict(gains=[None, None]), dict(bad_constant=(70000, 15)),
               dict(bad_constant=(5, 0)), dict(bad_sites=[[1, 2]])):
        with pytest.raises(InvalidOptionError):
            dng.SiteCorrections(**kw)
    for nodes in ([[16.0]], [[-0.1]], [[np.nan]], np.ones((1, 4097))):
        with pytest.raises(InvalidOptionError):
            dng.GainMap(nodes)
    sc = dng.SiteCorrections(black_h=[0, 1, 2], bad_sites=[7], bad_constant=(300, 15))
    with pytest.raises(InvalidOptionError):
        sc.quantised((2, 4), np.uint16)         # three column deltas for four columns
    with pytest.raises(InvalidOptionError):
        dng.SiteCorrections(bad_sites=[7]).quantised((2, 3), np.uint16)      # the site lies outside
    with pytest.raises(InvalidOptionError):
        dng.SiteCorrections(bad_constant=(300, 15)).quantised((2, 3), np.uint8)
    for bad in ("yes", 3):
        with pytest.raises(InvalidOptionError):
            dng.Raw(corrections=bad)
    assert dng.Raw().corrections is None and dng.Raw(corrections="auto").corrections == "auto"
    assert repr(dng.Raw()) == "Raw(develop='auto', lens='auto', calibration=None)"


# ------------------------------------------------------------------------------------------------ the parser
H, W = 21, 37
NODES = {p: SC.f32(SC._nodes(mv, mh, 20 + p)) for p, (mv, mh) in enumerate(((2, 3), (3, 2), (1, 4), (4, 4)))}


def _four_maps():
    """one GainMap opcode per position: pitch 2, the rectangle starting on the position's first site"""
    return [SC.gain_map_opcode(NODES[p], (p >> 1, p & 1, H, W), pitch=(2, 2)) for p in range(4)]


def _write(tmp_path, name, opcodes2=None, extra=None, bits=12, **kw):
    stored = np.random.default_rng(5).integers(0, 1 << bits, size=(H, W))
    path = str(tmp_path / name)
    DC.write_dng(path, stored, bits, opcodes2=opcodes2, extra=extra, **kw)
    return dng.read(path)


def test_parser_reads_maps_deltas_and_bad_sites(tmp_path):
    dh = [0.25 * (x % 5) - 0.5 for x in range(W)]
    dv = [0.5 - 0.125 * (y % 3) for y in range(H)]
    ops = _four_maps() + [SC.bad_list_opcode(points=[(3, 4), (20, 36), (50, 2)], rects=[(5, 6, 8, 9), (19, 35, 40, 40)]),
                          SC.bad_constant_opcode(4095)]
    frame = _write(tmp_path, "all.dng", ops, black=(64, 64, 64, 64),
                   extra={50715: (10, [DC.rational(v) for v in dh]), 50716: (10, [DC.rational(v) for v in dv])})
    c = frame.corrections
    assert c is not None and c.skipped == ()
    shift = frame.layout.shift
    assert shift == 4
    assert c.black_h.tolist() == [int(np.floor(v * 16 + 0.5)) for v in dh]
    assert c.black_v.tolist() == [int(np.floor(v * 16 + 0.5)) for v in dv]
    for p in range(4):
        assert np.array_equal(c.gains[p].nodes, NODES[p])
        mv, mh = NODES[p].shape
        assert c.gains[p].spacing == (1.0 / max(mv - 1, 1), 1.0 / max(mh - 1, 1)) and c.gains[p].origin == (0.0, 0.0)
    want = {3 * W + 4, 20 * W + 36} | {y * W + x for y in range(5, 8) for x in range(6, 9)} | {y * W + x for y in (19, 20) for x in (35, 36)}
    assert c.bad_sites.dtype == np.int32 and c.bad_sites.tolist() == sorted(want)
    assert c.bad_constant == (4095 << shift, 15)
    # `ignored` is what a default Raw() does not apply: all of it; `remaining` is what is left with the corrections
    assert frame.ignored == ("BlackLevelDeltaH", "BlackLevelDeltaV", "OpcodeList2", "GainMap", "GainMap", "GainMap", "GainMap",
                             "FixBadPixelsList", "FixBadPixelsConstant")
    assert frame.remaining() == frame.remaining(c) == ()
    assert frame.remaining(None) == frame.ignored
    assert frame.remaining(dng.SiteCorrections(black_h=c.black_h)) == frame.ignored[1:]
    # a pitch of 1 maps every position with one object
    frame = _write(tmp_path, "one.dng", [SC.gain_map_opcode(NODES[3], (0, 0, H, W)), (7, b"\0" * 8)])
    c = frame.corrections
    assert all(g is c.gains[0] for g in c.gains) and c.applies == ("GainMap",) and not c.whole_list2
    assert frame.remaining() == ("OpcodeList2", "MapTable")
    # a file without any of it
    assert _write(tmp_path, "none.dng").corrections is None


SKIPS = [
    ("zero points", DC.GAIN_MAP, "zero map points"),
    ("nan", SC.gain_map_opcode([[1.0, float("nan")]], (0, 0, H, W)), "not finite"),
    ("negative", SC.gain_map_opcode([[1.0, -0.5]], (0, 0, H, W)), "negative"),
    ("16", SC.gain_map_opcode([[1.0, 16.0]], (0, 0, H, W)), "16 or more"),
    ("rectangle", SC.gain_map_opcode([[1.0, 1.5]], (0, 0, H - 3, W)), "does not span"),
    ("rectangle start", SC.gain_map_opcode([[1.0, 1.5]], (2, 0, H, W), pitch=(2, 2)), "does not span"),
    ("pitch", SC.gain_map_opcode([[1.0, 1.5]], (0, 0, H, W), pitch=(3, 1)), "pitch of 1 or 2"),
    ("planes", SC.gain_map_opcode([[1.0, 1.5]], (0, 0, H, W), planes=3), "one plane"),
    ("map planes", SC.gain_map_opcode([[1.0, 1.5]], (0, 0, H, W), map_planes=3), "one plane"),
    ("short body", SC.gain_map_opcode([[1.0, 1.5]], (0, 0, H, W), cut=3), "shorter than its 1 x 2 map points"),
    ("short header", (9, b"\0" * 40), "shorter than its 76-byte header"),
    ("list too long", SC.bad_list_opcode(rects=[(0, 0, 1024, 1025)]), "at most 2^20"),
    ("list short", (5, SC.bad_list_opcode(points=[(1, 1)])[1][:-2]), "shorter than its 1 points"),
    ("constant outside", SC.bad_constant_opcode(5000), "outside the samples' range"),
]


@pytest.mark.parametrize("what,opcode,reason", SKIPS, ids=[s[0] for s in SKIPS])
def test_an_opcode_that_cannot_be_used_is_skipped_with_its_reason(tmp_path, what, opcode, reason):
    # (the rectangle of the too-long list is clipped to the image only after it is counted: write a big image's worth)
    frame = _write(tmp_path, "skip.dng", [opcode])
    c = frame.corrections
    name = dng.OPCODE_NAMES[opcode[0]]
    assert c is not None and c.empty and len(c.skipped) == 1
    assert c.skipped[0][0] == name and reason in c.skipped[0][1], c.skipped
    assert frame.ignored == ("OpcodeList2", name) and frame.remaining() == frame.ignored


def test_more_skips_second_map_deltas_table(tmp_path):
    # a second map for a position: the first holds
    ops = [SC.gain_map_opcode(NODES[0], (0, 0, H, W)), SC.gain_map_opcode(NODES[1], (1, 1, H, W), pitch=(2, 2))]
    c = _write(tmp_path, "second.dng", ops).corrections
    assert c.skipped == (("GainMap", "a second map for position 3"),) and np.array_equal(c.gains[3].nodes, NODES[0])
    assert c.applies == ("GainMap",)
    # deltas of the wrong count; deltas that drive black + delta out of range
    frame = _write(tmp_path, "count.dng", extra={50715: (10, [DC.rational(0.0)] * (W - 1))})
    assert frame.corrections.empty and "36 entries for a crop of 37 columns" in frame.corrections.skipped[0][1]
    assert frame.ignored == ("BlackLevelDeltaH",) == frame.remaining()
    frame = _write(tmp_path, "range.dng", black=(2, 2, 2, 2),
                   extra={50716: (10, [DC.rational(-3.0)] * H), 50715: (10, [DC.rational(0.0)] * W)})
    assert frame.corrections.empty and [n for n, _ in frame.corrections.skipped] == ["BlackLevelDeltaH", "BlackLevelDeltaV"]
    assert "outside [0, 65535]" in frame.corrections.skipped[0][1]
    # FixBadPixelsConstant beside a LinearizationTable
    frame = _write(tmp_path, "table.dng", [SC.bad_constant_opcode(0)], table=list(range(4096)))
    assert frame.corrections.empty and "LinearizationTable" in frame.corrections.skipped[0][1]
    assert frame.ignored == ("OpcodeList2", "FixBadPixelsConstant")


def test_the_existing_zero_body_gain_map_file_still_reads(tmp_path):
    case = DC.BY_NAME["14bit-colour-rational-black"]
    case.write(str(tmp_path / "a.dng"))
    frame = dng.read(str(tmp_path / "a.dng"))
    assert frame.ignored == ("BlackLevelDeltaH", "DefaultCropOrigin", "DefaultCropSize", "AnalogBalance", "OpcodeList2", "GainMap", "GainMap")
    c = frame.corrections
    assert c.skipped == (("GainMap", "zero map points"),)
    assert c.black_h.tolist() == [0] * 10 and c.applies == ("BlackLevelDeltaH",)
    assert frame.remaining() == frame.ignored[1:]
    for name, other in DC.BY_NAME.items():
        if "opcodes2" not in other.kw and not any(t in other.kw.get("extra", {}) for t in (50715, 50716)):
            other.write(str(tmp_path / "b.dng"))
            assert dng.read(str(tmp_path / "b.dng")).corrections is None, name
