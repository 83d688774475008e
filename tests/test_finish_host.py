"""CPU: the host half of the finish (dng.RadialGain, dng.Finish, the parser) and the cases of tests/finish_cases.py.

No case is vacuous (the predictor says each reaches the path it is named for); the orientation table is Pillow's; the quantised
gain lies within the derived bound of the float64 polynomial; the warp-inverted table equals a direct float64 evaluation; the
parser reads what the writer wrote, skips what it must with a reason, and `remaining` / `finished_shape` follow; the default
Raw() touches nothing."""
import math
import struct

import numpy as np
import pytest

import dng_cases as DC
import finish_cases as FC
import finish_restatement as R
from shinestacker_amd import InvalidOptionError, Lens, dng


# ------------------------------------------------------------------------------------------------ the cases mean something
def test_every_radial_case_reaches_the_path_it_is_named_for():
    seen = {c.name: FC.radial_paths(c) for c in FC.RADIAL_CASES}
    assert set().union(*seen.values()) == set(FC.RADIAL_PATHS)
    for name, p in seen.items():
        if "2x2" in name:
            assert p <= {"partial", "misaligned row"} and "partial" in p, (name, p)
        if "2x37" in name:
            assert {"whole", "partial", "misaligned row"} <= p, (name, p)
        if "one-span" in name:
            assert p == {"whole"}, (name, p)              # 64 whole windows a row and nothing else
        if "below-a-span" in name:
            assert {"whole", "partial", "misaligned row"} <= p, (name, p)
        if "above-a-span" in name:
            assert {"whole", "partial", "second workgroup"} <= p, (name, p)
        if "rows-off-the-grid" in name:
            assert "misaligned row" in p, (name, p)
    for dt in (np.uint8, np.uint16):        # both dtypes see every path, both kinds of centre and of gain
        mine = [c for c in FC.RADIAL_CASES if c.dtype == dt]
        assert set().union(*(seen[c.name] for c in mine)) == set(FC.RADIAL_PATHS)
        assert any(c.k == FC.VIG_SATURATE for c in mine) and any(c.k == FC.VIG_DARKEN for c in mine)
        assert any(not (0 <= c.centre[0] < c.w and 0 <= c.centre[1] < c.h) for c in mine)
    assert any(c.centre == (0.0, 0.0) for c in FC.RADIAL_CASES)
    # "saturates" and "darkens" do what they say, by the restatement
    for c in FC.RADIAL_CASES:
        g = dng.RadialGain(c.k, c.centre)
        out = R.radial_gain(c.mosaic(), c.black, *g.centre2(), g.table())
        top = int(np.iinfo(c.dtype).max)
        if "saturates" in c.name:
            assert ((out == top) & (c.mosaic() < top)).sum() > c.h * c.w // 4, c
        if "darkens" in c.name:
            above = c.mosaic().astype(int) > np.asarray(c.black)[2 * (np.arange(c.h)[:, None] & 1) + (np.arange(c.w)[None, :] & 1)]
            assert (out.astype(int)[above] <= c.mosaic().astype(int)[above]).all() and (out != c.mosaic()).any(), c


def test_every_finish_case_reaches_the_path_it_is_named_for():
    union = set()
    for c in FC.FINISH_CASES:
        for dt in (np.uint8, np.uint16):
            for o in FC.ORIENTATIONS:
                p = FC.finish_paths(c, dt, o)
                union |= p
                assert p, (c, dt, o)
                if "tile-edge" in c.name and o >= 5:
                    assert "tile edge" in p, (c, p)
                if "one-tile" in c.name and o >= 5:
                    assert p == {"tile interior"}, (c, p)
                if "tiles-down" in c.name and o >= 5:
                    assert p == {"tile interior", "tile edge"}, (c, p)
                if "crop-odd-origin" in c.name and o < 5:
                    assert {"whole", "partial", "misaligned row"} <= p and (("misaligned source" in p) == (o in (1, 4))), (c, o, p)
                if "two-workgroups" in c.name and o < 5:
                    assert "second workgroup" in p, (c, p)
                if "64-wide" in c.name and o in (1, 4) and dt == np.uint8:
                    assert p == {"whole"}, (c, p)          # rows and sources on the grid: nothing but whole windows
                if c.name in ("1x1", "40x50-crop-to-1x1"):
                    assert p == ({"partial"} if o < 5 else {"tile edge"}), (c, p)
    assert union == set(FC.FINISH_PATHS)
    for dt in (np.uint8, np.uint16):        # every instantiation of the flipped window, at each dtype
        flipped = set().union(*(FC.finish_paths(c, dt, o) for c in FC.FINISH_CASES for o in (2, 3)))
        assert {"flip phase 0", "flip phase 1", "flip phase 2"} <= flipped, (dt, flipped)
    shapes =[c.rect()[2:] for c in FC.FINISH_CASES]
    assert any(h != w for h, w in shapes) and (1, 1) in shapes and any(h == 1 < w for h, w in shapes) and any(w == 1 < h for h, w in shapes)
    for edge in (FC.TILE - 1, FC.TILE, FC.TILE + 1):
        assert any(h == edge for h, _ in shapes) and any(w == edge for _, w in shapes)


# ------------------------------------------------------------------------------------------------ orientation
def test_the_orientation_table_is_pillows():
    """the mapping ImageOps.exif_transpose uses, on a frame that is not square"""
    from PIL import Image
    T = getattr(Image, "Transpose", Image)
    method = {2: T.FLIP_LEFT_RIGHT, 3: T.ROTATE_180, 4: T.FLIP_TOP_BOTTOM, 5: T.TRANSPOSE, 6: T.ROTATE_270, 7: T.TRANSVERSE, 8: T.ROTATE_90}
    a = np.random.default_rng(3).integers(0, 256, size=(5, 7, 3)).astype(np.uint8)
    img = Image.fromarray(a)
    assert np.array_equal(R.finish(a, None, 1), a)
    for o, m in method.items():
        want = np.asarray(img.transpose(m))
        got = R.finish(a, None, o)
        assert got.shape == want.shape and np.array_equal(got, want), o
        assert dng.Finish(orientation=o).finished_shape(a.shape[:2]) == want.shape[:2]
        cropped = R.finish(a, (1, 2, 3, 4), o)
        assert np.array_equal(cropped, np.asarray(Image.fromarray(np.ascontiguousarray(a[1:4, 2:6])).transpose(m))), o
        assert dng.Finish(crop=(1, 2, 3, 4), orientation=o).finished_shape(a.shape[:2]) == cropped.shape[:2]


# ------------------------------------------------------------------------------------------------ the quantised gain
def _exact_u(h, w, centre):
    cx, cy = centre
    d2 = (np.arange(w)[None, :] - cx) ** 2 + (np.arange(h)[:, None] - cy) ** 2
    return d2 / max((x - cx) ** 2 + (y - cy) ** 2 for x in (0, w - 1) for y in (0, h - 1))


@pytest.mark.parametrize("case", FC.RADIAL_CASES, ids=repr)
def test_the_quantised_gain_lies_within_the_derived_bound(case):
    g = dng.RadialGain(case.k, case.centre)
    cx2, cy2 = g.centre2()
    assert abs(cx2 / 2 - case.centre[0]) <= 0.25 and abs(cy2 / 2 - case.centre[1]) <= 0.25
    table = g.table()
    assert table.dtype == np.uint16 and table.shape == (R.NODES,) and table.max() < 65535      # (the clamp is not in play)
    got = R.radial_g(case.h, case.w, cx2, cy2, table) / 4096.0
    bound = R.gain_error_bound(case.k, case.h, case.w, cx2, cy2)
    err = np.abs(got - g.gain(_exact_u(case.h, case.w, case.centre))).max()
    assert err <= bound, (case, err, bound)
    # about the half-pixel centre itself the centre's term is gone: what is left is table, format and weight
    exact = dng.RadialGain(case.k, (cx2 / 2, cy2 / 2))
    assert exact.centre2() == (cx2, cy2)
    sharp = R.gain_error_bound(case.k, case.h, case.w, cx2, cy2, centre_exact=True)
    err = np.abs(got - exact.gain(_exact_u(case.h, case.w, exact.centre))).max()
    assert err <= sharp < 6e-4, (case, err, sharp)


def test_the_multiplier_and_shift_stand_in_for_the_division():
    for D in (1, 2, 3, 4, 1000, 7741, 2 ** 20 + 1, 2 ** 39 + 12345, 2 ** 40 - 1):
        mul, shift = R.radial_map(D)
        assert 2 ** 23 <= mul < 2 ** 24 and 0 <= shift <= 46, (D, mul, shift)
        for d2 in {0, 1, D // 3, D // 2, D - 1, D}:
            q = (d2 * mul) >> shift
            assert d2 * mul < 2 ** 64 and q <= R.Q_ONE and 0 <= d2 * R.Q_ONE / D - q < 1 + 1 / 32, (D, d2, q)
    assert dng.radial_d2max(21, 40, 7, -3) == R.d2max(21, 40, 7, -3) == (2 * 39 - 7) ** 2 + (2 * 20 + 3) ** 2


# ------------------------------------------------------------------------------------------------ the warp's inverse
BARREL = Lens.distortion(-0.08, 0.01)


def _solve(lens_k, u_src):
    """u_dst with u_dst s(u_dst)^2 = u_src by bisection (the map is increasing), clamped to [0, 1]"""
    k0, k1, k2, k3 = lens_k

    def fwd(u):
        s = ((k3 * u + k2) * u + k1) * u + k0
        return u * s * s
    if fwd(1.0) <= u_src:
        return 1.0
    lo, hi = 0.0, 1.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if fwd(mid) < u_src else (lo, mid)
    return 0.5 * (lo + hi)


def test_the_warp_inverted_table_equals_a_direct_evaluation():
    """table(u_src) = g(u_dst(u_src)) at every node: u_dst by bisection here, by interpolation over 2^16 intervals there -- the
    two lie within one interval, 2^-16, so the nodes agree within half a Q12 step plus max|g'| 2^-16"""
    g = dng.RadialGain(FC.VIG, (30.0, 20.0), after_warp=True)
    table = g.table(BARREL)
    g1 = sum((i + 1) * abs(k) for i, k in enumerate(FC.VIG))
    want = np.array([float(g.gain(_solve(BARREL.k[1], i / 1024.0))) for i in range(R.NODES)])
    assert np.abs(table / 4096.0 - want).max() <= 2.0 ** -13 + g1 * 2.0 ** -16
    # the barrel lens pulls sources inward: the corner's source lies inside the frame, and beyond it the corner's gain holds
    assert _solve(BARREL.k[1], 0.9) == 1.0 and table[-1] == table[1000] == math.floor(4096 * 1.4 + 0.5)
    # sources inside: the gain is read further out everywhere; near the centre the difference is below a Q12 step
    assert (table >= g.table()).all() and (table[512:-1] > g.table()[512:-1]).all()
    # not after a warp, or no lens applied: the polynomial itself
    assert np.array_equal(dng.RadialGain(FC.VIG, (30.0, 20.0)).table(BARREL), g.table())
    assert np.array_equal(g.table(None), np.floor(4096 * g.gain(np.arange(1025) / 1024.0) + 0.5).astype(np.uint16))
    with pytest.raises(InvalidOptionError, match="monotone"):
        g.table(Lens.distortion(-2.0))


def test_the_gain_error_of_ignoring_lateral_ca_is_bounded():
    """red and blue get green's table.  Under the largest CA the tests write (planes 1.01 / 1.0 / 0.99) u_dst of a site is off by
    at most du = max |u_dst,plane - u_dst,green| and the gain by at most max|g'| du: the figure of RadialGain's docstring"""
    ca = Lens(((0.99, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.01, 0.0, 0.0, 0.0)))
    g = dng.RadialGain(FC.VIG, (30.0, 20.0), after_warp=True)
    us = np.linspace(0.0, 1.0, 513)
    green = np.array([_solve(ca.k[1], u) for u in us])
    du = max(np.abs(np.array([_solve(k, u) for u in us]) - green).max() for k in (ca.k[0], ca.k[2]))
    g1 = sum((i + 1) * abs(k) for i, k in enumerate(FC.VIG))
    worst = max(np.abs(g.gain(np.array([_solve(k, u) for u in us])) - g.gain(green)).max() for k in (ca.k[0], ca.k[2]))
    assert du <= 0.0204 and worst <= g1 * du <= 0.0102
    assert "0.0102" in dng.RadialGain.__doc__


# ------------------------------------------------------------------------------------------------ the parser
H, W = 24, 40


def _write(tmp_path, name="f.dng", **kw):
    p = str(tmp_path / name)
    stored = np.random.default_rng(1).integers(0, 4096, size=(H, W))
    base = dict(black=(256,), neutral=(0.55, 1.0, 0.7), matrices={1: (DC.XYZ_D65_MATRIX, 21)})
    base.update(kw)
    DC.write_dng(p, stored, 12, **base)
    return dng.read(p)


@pytest.mark.parametrize("typ", [3, 4, 5], ids=["SHORT", "LONG", "RATIONAL"])
def test_the_parser_reads_what_the_writer_wrote(tmp_path, typ):
    f = _write(tmp_path, opcodes3=[DC.WARP, FC.fix_vignette_radial(FC.VIG5, (0.5, 0.5))], orientation=6,
               extra=FC.default_crop((6, 2), (30, 19), typ))
    fin = f.finish
    assert isinstance(fin, dng.Finish) and fin.skipped == () and not fin.empty
    assert fin.vignette.k == FC.VIG5 and fin.vignette.centre == (0.5 * (W - 1), 0.5 * (H - 1)) and fin.vignette.after_warp
    assert fin.crop == (2, 6, 19, 30) and fin.orientation == f.orientation == 6        # (y, x, h, w) from (horizontal, vertical)
    assert fin.applies == ("FixVignetteRadial", "DefaultCropOrigin", "DefaultCropSize")
    assert f.finished_shape() == f.finished_shape("auto") == (30, 19) and f.finished_shape(None) == f.shape == (H, W)
    assert f.finished_shape(dng.Finish(orientation=3)) == (H, W) and f.finished_shape(dng.Finish(crop=(0, 0, 5, 7), orientation=8)) == (7, 5)
    assert sorted(f.ignored) == sorted(["DefaultCropOrigin", "DefaultCropSize", "FixVignetteRadial"])
    assert f.remaining() == f.remaining(finish=None) == f.ignored
    assert f.remaining(finish="auto") == () == f.remaining(corrections="auto", finish="auto")
    assert f.remaining(finish=dng.Finish(crop=(0, 0, 4, 4))) == ("FixVignetteRadial",)
    # no warp in front of it: the polynomial stands as it is; a centre off the middle is placed as the warp's is
    f = _write(tmp_path, opcodes3=[FC.fix_vignette_radial(FC.VIG, (0.25, 0.75))])
    assert not f.finish.vignette.after_warp and f.finish.vignette.centre == (0.25 * (W - 1), 0.75 * (H - 1))
    assert f.finish.crop is None and f.finish.orientation == 1 and f.remaining(finish="auto") == ()
    # a size alone: the origin is (0, 0)
    f = _write(tmp_path, extra={50720: (4, [10, 8])})
    assert f.finish.crop == (0, 0, 8, 10) and f.finish.applies == ("DefaultCropSize",) and f.remaining(finish="auto") == ()


def test_a_file_without_any_of_it_has_an_empty_finish(tmp_path):
    f = _write(tmp_path)
    assert f.finish.empty and f.finish.skipped == () and f.finished_shape() == f.shape
    assert dng.resolve_finish(f, "auto") is None and dng.Raw(finish="auto").finish_for(f) is None
    f = _write(tmp_path, orientation=1)
    assert f.finish.empty


SKIPS = {
    "short body": (dict(opcodes3=[(3, struct.pack(">6d", 0.1, 0, 0, 0, 0, 0.5))]), "shorter than its seven doubles"),
    "coefficient not finite": (dict(opcodes3=[FC.fix_vignette_radial((0.1, float("nan"), 0, 0, 0), (0.5, 0.5))]), "not finite"),
    "centre not finite": (dict(opcodes3=[FC.fix_vignette_radial(FC.VIG, (float("inf"), 0.5))]), "not finite"),
    "gain not positive": (dict(opcodes3=[FC.fix_vignette_radial((-2.0, 0, 0, 0, 0), (0.5, 0.5))]), "inside (0, 16)"),
    "gain of 16 or more": (dict(opcodes3=[FC.fix_vignette_radial((15.0, 0, 0, 0, 0), (0.5, 0.5))]), "inside (0, 16)"),
    "a second one": (dict(opcodes3=[FC.fix_vignette_radial(FC.VIG, (0.5, 0.5)), FC.fix_vignette_radial(FC.VIG5, (0.5, 0.5))]), "second FixVignetteRadial"),
    "before the warp": (dict(opcodes3=[FC.fix_vignette_radial(FC.VIG, (0.5, 0.5)), DC.WARP]), "before the WarpRectilinear"),
    "default scale": (dict(opcodes3=[FC.fix_vignette_radial(FC.VIG, (0.5, 0.5))], extra=FC.default_scale(1.0, 1.5)), "DefaultScale"),
    "another centre than the warp's": (dict(opcodes3=[DC.WARP, FC.fix_vignette_radial(FC.VIG, (0.4, 0.5))]), "is not the WarpRectilinear's"),
    "warp not monotone": (dict(opcodes3=[DC.warp_rectilinear([(1.0, -2.0, 0.0, 0.0, 0.0, 0.0)], (0.5, 0.5)),
                                         FC.fix_vignette_radial(FC.VIG, (0.5, 0.5))]), "not monotone"),
}


@pytest.mark.parametrize("why", sorted(SKIPS))
def test_a_vignette_that_cannot_be_used_is_skipped_with_its_reason(tmp_path, why):
    kw, reason = SKIPS[why]
    f = _write(tmp_path, **kw)
    assert f.finish.vignette is None and "FixVignetteRadial" not in f.finish.applies
    assert any(n == "FixVignetteRadial" and reason in r for n, r in f.finish.skipped), f.finish.skipped
    assert "FixVignetteRadial" in f.ignored and "FixVignetteRadial" in f.remaining(finish="auto")


CROP_SKIPS = {
    "not integral": (FC.default_crop((2.5, 2), (30, 19), 5), "not integral"),
    "outside the frame": (FC.default_crop((12, 2), (30, 19)), "lies outside the 24 x 40 frame"),
    "empty": (FC.default_crop((0, 0), (0, 19)), "lies outside"),
    "origin alone": ({50719: (4, [2, 2])}, "without a DefaultCropSize"),
}


@pytest.mark.parametrize("why", sorted(CROP_SKIPS))
def test_a_crop_that_cannot_be_used_is_skipped_with_its_reason(tmp_path, why):
    extra, reason = CROP_SKIPS[why]
    f = _write(tmp_path, extra=extra)
    assert f.finish.crop is None and f.finish.empty and f.finished_shape() == f.shape
    names = [n for n in ("DefaultCropOrigin", "DefaultCropSize") if n in f.ignored]
    assert names and sorted(n for n, r in f.finish.skipped if reason in r) == sorted(names), f.finish.skipped
    assert f.remaining(finish="auto") == f.ignored


def test_an_orientation_outside_1_to_8_is_refused(tmp_path):
    for bad in (0, 9):
        with pytest.raises(InvalidOptionError, match=f"Orientation.*{bad}"):
            _write(tmp_path, orientation=bad)
    for o in range(1, 9):
        assert _write(tmp_path, orientation=o).finish.orientation == o


def test_remaining_with_corrections_and_a_finish(tmp_path):
    """a file carrying the three items beside site corrections: each option removes its own and nothing else"""
    gm = struct.pack(">10I4dI", 0, 0, H, W, 0, 1, 1, 1, 1, 1, 1.0, 1.0, 0.0, 0.0, 1) + struct.pack(">f", 1.25)
    f = _write(tmp_path, opcodes2=[(9, gm)], opcodes3=[DC.WARP, FC.fix_vignette_radial(FC.VIG, (0.5, 0.5))], orientation=8,
               extra={**FC.default_crop((2, 2), (36, 20)), 50727: (5, [DC.rational(1.0)] * 3)})
    assert sorted(f.ignored) == sorted(["AnalogBalance", "DefaultCropOrigin", "DefaultCropSize", "OpcodeList2", "GainMap", "FixVignetteRadial"])
    assert f.remaining(corrections=None) == f.ignored
    assert sorted(f.remaining()) == sorted(["AnalogBalance", "DefaultCropOrigin", "DefaultCropSize", "FixVignetteRadial"])   # (as before)
    assert sorted(f.remaining(corrections=None, finish="auto")) == sorted(["AnalogBalance", "OpcodeList2", "GainMap"])
    assert sorted(f.remaining(corrections="auto", finish=None)) == sorted(["AnalogBalance", "DefaultCropOrigin", "DefaultCropSize", "FixVignetteRadial"])
    assert f.remaining(corrections="auto", finish="auto") == ("AnalogBalance",)
    with pytest.raises(InvalidOptionError):
        f.remaining(finish="file")


# ------------------------------------------------------------------------------------------------ the objects
def test_radial_gain_and_finish_refuse_what_they_cannot_use():
    for k, c in (((0.1, 0, 0, 0), (1, 1)), ((0.1, 0, 0, 0, 0, 0), (1, 1)), ((0.1, 0, 0, 0, 0), (1,)), ("abcde", (1, 1)),
                 ((0.1, 0, 0, 0, float("nan")), (1, 1)), ((0.1, 0, 0, 0, 0), (float("inf"), 1)), ((-1.0, 0, 0, 0, 0), (1, 1)),
                 ((15.0, 0, 0, 0, 0), (1, 1)), ((0.1, 0, 0, 0, 0), (2.0 ** 24, 1))):
        with pytest.raises(InvalidOptionError):
            dng.RadialGain(k, c)
    g = dng.RadialGain(FC.VIG, (3.0, 2.0))
    with pytest.raises(InvalidOptionError, match="farthest corner"):
        dng.RadialGain(FC.VIG, (2.0 ** 22, 0.0)).check_shape((20, 30))
    assert g.check_shape((20, 30)) == (6, 4)
    for kw in (dict(vignette=FC.VIG), dict(crop=(1, 2, 3)), dict(crop=(1.0, 2, 3, 4)), dict(crop=(-1, 0, 2, 2)), dict(crop=(0, 0, 0, 2)),
               dict(orientation=0), dict(orientation=9), dict(orientation=True), dict(orientation=2.0)):
        with pytest.raises(InvalidOptionError):
            dng.Finish(**kw)
    fin = dng.Finish(g, (1, 2, 3, 4), 5)
    assert fin.finished_shape((10, 12)) == (4, 3) and fin.crop_for((10, 12)) == (1, 2, 3, 4) and fin.geometry((10, 12))
    with pytest.raises(InvalidOptionError, match="outside the 3 x 12 frame"):
        fin.finished_shape((3, 12))
    assert not dng.Finish(g).geometry((10, 12)) and not dng.Finish(crop=(0, 0, 10, 12)).geometry((10, 12))
    assert dng.Finish().empty and not dng.Finish(g).empty and not dng.Finish(orientation=2).empty
    for bad in ("file", 3, FC.VIG):
        with pytest.raises(InvalidOptionError):
            dng.Raw(finish=bad)
    assert dng.Raw(finish=fin).finish is fin and "finish=" in repr(dng.Raw(finish="auto")) and "finish" not in repr(dng.Raw())


def test_the_default_raw_applies_nothing(tmp_path):
    """finish= is off unless asked for: Raw() resolves to no finish on a file that carries all three, `ignored` lists them as
    before, and the shape a stack is created with is the stored frame's"""
    f = _write(tmp_path, opcodes3=[FC.fix_vignette_radial(FC.VIG, (0.5, 0.5))], orientation=6, extra=FC.default_crop((2, 2), (36, 20)))
    raw = dng.Raw()
    assert raw.finish is None and raw.finish_for(f) is None and dng.resolve_finish(f, None) is None
    assert sorted(f.ignored) == sorted(["DefaultCropOrigin", "DefaultCropSize", "FixVignetteRadial"]) and f.orientation == 6
    assert f.shape == (H, W) and f.finished_shape(None) == (H, W)
    assert dng.Raw(finish="auto").finish_for(f) is f.finish and f.finished_shape() == (36, 20)
    # the existing table: every case parses, `ignored` of the one that carries a crop is what it was
    c = DC.BY_NAME["14bit-colour-rational-black"]
    c.write(str(tmp_path / "c.dng"))
    f = dng.read(str(tmp_path / "c.dng"))
    assert sorted(f.ignored) == sorted(["BlackLevelDeltaH", "AnalogBalance", "DefaultCropOrigin", "DefaultCropSize", "OpcodeList2",
                                        "GainMap", "GainMap"])
    assert f.finish.crop == (0, 0, 6, 10) and not f.finish.geometry(f.shape)
