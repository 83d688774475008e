"""CPU: the cases of tests/balance_cases.py mean something.  The grid caps the "long grid" cases are sized against are the
ones written in csrc/capi.hip (a changed cap fails here, it does not silently un-test a grid-stride loop); the cube holds
every colour once and the oracle maps hue 180..255 to hue 0; the histogram cases have the partial blocks, the dropped
blocks and the points on the mask's circle they are named for; balance_cases.linear_table, the restatement of
lut_linear_build, equals the host class LinearMap and the reference's recorded LINEAR tables."""
import json
import os
import re
import warnings

import numpy as np
import pytest

import balance_cases as B
from conftest import ROOT, load_golden

CSRC = os.path.join(ROOT, "shinestacker_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_grid_caps_match_the_launchers():
    capi, kern = _source("capi.hip"), _source("kernels_balance.hpp")
    hist = re.findall(r"std::min<size_t>\(\(total \+ 255\) / 256, (\d+) \* (\d+)\)", capi)
    lut = re.findall(r"std::min<size_t>\(\(n / (\d+) \+ 255\) / 256 \+ 1, (\d+) \* (\d+)\)", capi)
    cvt = re.findall(r"std::min<size_t>\(\(npixels \+ 255\) / 256, (\d+) \* (\d+)\)", capi)
    assert len(hist) == 1 and len(lut) == 1 and len(cvt) == 1, "a launcher of the balance kernels sizes its grid another way"
    assert int(hist[0][0]) * int(hist[0][1]) == B.HIST_MAX_BLOCKS
    assert int(lut[0][0]) == B.LUT_U8_PER_THREAD and int(lut[0][1]) * int(lut[0][2]) == B.LUT_MAX_BLOCKS
    assert int(cvt[0][0]) * int(cvt[0][1]) == B.CVT_MAX_BLOCKS
    # every launch of the family is 256 wide, and lut_apply_u8 steps by the 12 bytes the launcher counts with
    for kernel in ("hist_u8", "hist_u16", "lut_apply_u8", "lut_apply_u16"):
        assert re.search(r"hipLaunchKernelGGL\(%s, dim3\(nblk\), dim3\((\d+)\)" % kernel, capi).group(1) == str(B.BLOCK)
    assert re.search(r"mi_cvt_color_device.*?blk\((\d+)\);", capi, re.S).group(1) == str(B.BLOCK)
    assert re.search(r"const size_t nq = n / (\d+);", kern).group(1) == str(B.LUT_U8_PER_THREAD)
    assert (B.HIST_CAP, B.LUT_U8_CAP, B.LUT_U16_CAP, B.CVT_CAP) == (524288, 12582912, 1048576, 1048576)


def test_long_grid_cases_exceed_the_caps():
    h, w = B.LONG_LUT_SHAPE[np.uint8]
    assert h * w * 3 == 12607500 and h * w * 3 // B.LUT_U8_PER_THREAD > B.LUT_MAX_BLOCKS * B.BLOCK   # whole steps past one pass
    assert (h * w * 3) % 4 == 0          # the whole frame is dwords: no tail hides a missing step
    h, w = B.LONG_LUT_SHAPE[np.uint16]
    assert h * w * 3 == 1080000 > B.LUT_U16_CAP
    for case in B.LONG_HIST_CASES:
        hs, ws = B.subsampled_size(*case.shape, case.s, case.fast)
        assert (hs, ws) == (725, 730) and hs * ws == 529250 > B.HIST_CAP and not case.fast
    assert B.CUBE_SIDE * B.CUBE_SIDE == 1 << 24 > B.CVT_CAP
    assert B.LONG_HIST_CASES[1].mask == 0.9 and B.LONG_HIST_CASES[0].mask == 0.0


def test_cube_holds_every_colour_once():
    c = B.cube()
    assert c.shape == (4096, 4096, 3) and c.dtype == np.uint8 and not c.flags.writeable
    key = (c[..., 0].astype(np.uint32) << 16) | (c[..., 1].astype(np.uint32) << 8) | c[..., 2]
    assert np.array_equal(key.reshape(-1), np.arange(1 << 24, dtype=np.uint32))
    slabs = B.cube_slabs()
    assert len(slabs) == 256 // B.CUBE_SLAB and slabs[0][0] == 0 and slabs[-1][1] == B.CUBE_SIDE
    for k, (y0, y1) in enumerate(slabs):
        ch0 = c[y0:y1, :, 0]
        assert ch0.min() == k * B.CUBE_SLAB and ch0.max() == (k + 1) * B.CUBE_SLAB - 1
        assert y0 == (slabs[k - 1][1] if k else 0)


@pytest.mark.parametrize("code", [1, 3], ids=["hsv2bgr", "hls2bgr"])
def test_oracle_maps_hue_180_to_255_to_hue_0(oracle, code):
    """both inverse conversions: a hue past the 8-bit range [0, 180) gives the colour of hue 0 at the same other two channels
    -- and hue 0 is not what a hue folded by % 180 gives, so a test that folds never sees the branch"""
    c = B.cube()
    rows0 = c[:16]                                           # hue 0: every pair of the other two channels
    assert rows0[..., 0].max() == 0 and rows0.shape[0] * rows0.shape[1] == 65536
    want = oracle.cvt_color_u8(rows0, code)
    folded_differs = 0
    for hue in (180, 181, 209, 210, 239, 240, 254, 255):
        rows = c[16 * hue:16 * hue + 16]
        assert rows[..., 0].min() == hue == rows[..., 0].max() and np.array_equal(rows[..., 1:], rows0[..., 1:])
        assert np.array_equal(oracle.cvt_color_u8(rows, code), want), hue
        fold = rows.copy()
        fold[..., 0] = hue % 180
        folded_differs += int(hue % 180 != 0 and not np.array_equal(oracle.cvt_color_u8(fold, code), want))
    assert folded_differs == 7
    assert not np.array_equal(oracle.cvt_color_u8(c[16 * 179:16 * 180], code), want)     # 179 is still a hue of its own


@pytest.mark.parametrize("dtype", B.DTYPES, ids=B.dtype_name)
def test_histogram_cases_are_what_they_are_named_for(oracle, dtype):
    for case in B.HIST_CASES + B.LONG_HIST_CASES:
        h, w = case.shape
        hs, ws = B.subsampled_size(h, w, case.s, case.fast)
        assert B.hist_frame(case, dtype).shape == (h, w, 3) and not B.hist_frame(case, dtype).flags.writeable
        for lumi in (False, True):
            ref = B.hist_reference(oracle, case, dtype, lumi)
            assert ref.shape == (1 if lumi else 3, B.nbins_of(dtype)) and ref.dtype == np.int64
            if case.mask == 0.0:
                assert (ref.sum(axis=1) == hs * ws).all(), case
            else:
                assert (0 < ref.sum(axis=1)).all() and (ref.sum(axis=1) < hs * ws).all(), case
    by = {c.name: c for c in B.HIST_CASES}
    size = lambda n: B.subsampled_size(*by[n].shape, by[n].s, by[n].fast)
    assert size("1x1") == (1, 1) and size("2x2 area") == (1, 1) == size("2x2 fast")
    assert size("3x5 area") == (2, 2) and size("3x5 fast") == (2, 3) and size("5x7 area") == (2, 4) and size("7x9 fast s4") == (2, 3)
    assert size("121x152 area s3") == (40, 51)
    # kept partial blocks, and dropped ones
    partial = [c.name for c in B.HIST_CASES if B.has_partial_blocks(*c.shape, c.s, c.fast)]
    for name in ("3x5 area", "5x7 area", "121x152 area s3", "121x152 area s7", "119x154 area s3", "119x154 area s5", "119x154 area s6"):
        assert name in partial
    assert B.drops_last_block(3, 5, 2, False) and B.drops_last_block(5, 7, 2, False)
    c = by["119x154 area s5"]      # the corner block there is partial both ways: 4 x 4 of 5 x 5
    assert size(c.name) == (24, 31) and c.shape[0] - 23 * 5 == 4 and c.shape[1] - 30 * 5 == 4


def test_mask_cases_have_grid_points_exactly_on_the_circle(oracle):
    """so `<=` against `<` shows: the oracle's histogram with the boundary points left out is another histogram"""
    assert len(B.MASK_ON_CIRCLE) == 2
    for case in B.MASK_ON_CIRCLE:
        hs, ws = B.subsampled_size(*case.shape, case.s, case.fast)
        on = B.points_on_the_circle(hs, ws, case.mask)
        assert on == 2, case
        for dtype in B.DTYPES:
            ref = B.hist_reference(oracle, case, dtype, False)
            inside = oracle.balance_hist(B.hist_frame(case, dtype), False, case.s, case.fast, np.nextafter(case.mask, 0.0))
            assert (ref.sum(axis=1) - inside.sum(axis=1) == on).all()
    # the masks the older tests use put no point there
    for hs, ws, m in ((301, 453, 0.5), (64, 64, 0.95), (101, 151, 0.7), (250, 376, 0.95)):
        assert B.points_on_the_circle(hs, ws, m) == 0


@pytest.mark.parametrize("dtype", B.DTYPES, ids=B.dtype_name)
def test_area_results_at_odd_factors_differ_from_the_fast_ones(oracle, dtype):
    assert sorted({c.s for c in B.S_NOT_POWER_OF_TWO}) == [3, 5, 6, 7]
    for case in B.S_NOT_POWER_OF_TWO:
        img = B.hist_frame(case, dtype)
        for lumi in (False, True):
            area = B.hist_reference(oracle, case, dtype, lumi)
            fast = oracle.balance_hist(img, lumi, case.s, True, case.mask)
            assert area.shape == fast.shape and (area != fast).sum() > 20, case


def test_batch_and_table_cases():
    for dtype in B.DTYPES:
        a, b, c = B.batch_frames(dtype)
        assert a.shape == b.shape == c.shape == B.BATCH_SHAPE + (3,)
        assert not np.array_equal(a, c) and (b == B.vmax_of(dtype)).all()
        for nlut in (1, 3):
            ident, rep = B.lut_tables("identity", dtype, nlut), B.lut_tables("repeated", dtype, nlut)
            assert ident.shape == rep.shape == (nlut, B.nbins_of(dtype)) and ident.dtype == rep.dtype == np.dtype(dtype)
            assert (ident == np.arange(B.nbins_of(dtype))).all() and all(len(set(r.tolist())) == 1 for r in rep)
            assert len({int(r[0]) for r in rep}) == nlut
    tails = sorted({(h * w * 3) % 12 for h, w in B.LUT_SHAPES})
    assert tails == [0, 3, 6, 9]
    assert sum(h * w < 4 for h, w in B.LUT_SHAPES) == 3                      # only the tail runs
    assert {(h * w * 3) % 12 for h, w in B.LUT_SHAPES if h * w >= 4} == {0, 3, 6, 9}   # every tail behind whole steps too
    assert (B.LINEAR_SHAPE[0] * B.LINEAR_SHAPE[1] * 3) % 12 == 9


# ---------------------------------------------------------------- linear_table == LinearMap == the recording
def test_linear_table_equals_the_recorded_tables():
    g = load_golden("balance")
    seen = 0
    for m in json.loads(str(g["meta"])):
        if m["corr_map"] != "LINEAR":
            continue
        t, dtype = m["tag"], np.dtype(m["dtype"])
        n = B.nbins_of(dtype)
        iv = {"min": 0, "max": -1, **(m["opts"].get("intensity_interval") or {})}
        lo, hi = iv["min"], iv["max"] + 1 if iv["max"] >= 0 else n
        href, hmov = g[f"{t}_hist_ref"], g[f"{t}_hist_mov"]
        for c in range(len(href)):
            # the reference's mean of the reference frame, as _MeanMap states it; then the table from the moving frame's counts
            ref_mean = np.average(np.arange(n)[lo:hi], weights=href[c].reshape(-1)[lo:hi])
            table, ratio = B.linear_table(hmov[c], lo, hi, ref_mean, dtype)
            assert table.dtype == dtype and np.array_equal(table, g[f"{t}_luts"][c]), (m, c)
            assert ratio == np.asarray(g[f"{t}_size"], np.float64).ravel()[c], (m, c)
            seen += 1
    assert seen >= 8


@pytest.mark.parametrize("lumi", [True, False], ids=["lumi", "bgr"])
@pytest.mark.parametrize("dtype", B.DTYPES, ids=B.dtype_name)
def test_linear_table_equals_the_host_class(oracle, dtype, lumi):
    from shinestacker_amd.balance import LinearMap
    n = B.nbins_of(dtype)
    names = set()
    for case in B.linear_cases(dtype, lumi):
        frame, refs, tables, ratios, out = B.linear_expectation(oracle, case, dtype, lumi)
        names.add(case.name)
        assert tables.shape == ((1 if lumi else 3), n) and tables.dtype == np.dtype(dtype) and out.dtype == np.dtype(dtype)
        assert (tables[:case.first] == np.arange(n)).all()
        hist = oracle.balance_hist(frame, lumi, case.s, case.fast, case.mask)[case.first:]
        if case.name == "interval without counts":
            assert (hist[:, case.lo:case.hi] == 0).all() and (ratios == 1.0).all() and np.array_equal(out, frame)
            assert (tables == np.arange(n)).all()
            continue                                        # np.average raises there: the kernel's header defines the result
        cm = LinearMap(dtype, [h for h in hist], {"min": case.lo, "max": case.hi - 1})
        cm.reference = list(refs)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            corr = cm.correction([h for h in hist])
            host = np.stack([cm.table(c) for c in corr])
        assert np.array_equal(np.asarray(corr, np.float64), ratios, equal_nan=True), case
        assert np.array_equal(host, tables[case.first:]), case
        if case.name == "fifty times the mean":
            assert ((tables == n - 1).mean(axis=1) > 0.9).all()
        if case.name == "interval [1, 2)":
            assert (hist[:, 1] > 0).all() and np.allclose(ratios, refs)      # the mean over [1, 2) is 1
        if case.name == "black":
            assert np.isinf(ratios).all() and (tables[:, 0] == 0).all() and (tables[:, 1:] == n - 1).all() and not out.any()
        if case.name == "black, reference black":
            assert np.isnan(ratios).all() and not tables.any() and not out.any()
    assert {"random", "interval [1, 2)", "interval without counts", "fifty times the mean", "area s3 mask 0.8", "black"} <= names
    assert lumi or "first channel 1" in names
