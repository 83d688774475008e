"""CPU: the cases of tests/warp_cases.py, checked from the path predictor and oracle/align_oracle.c alone, so that the GPU
sweep over them (test_gpu_warp_edges.py) cannot pass on inputs that say nothing.  Everything asserted here is a condition on the
inputs: every `paths` case reaches the tile path in its name, the table as a whole reaches every class on ring and inner
tiles and thread-rows of both per-pixel kinds, `many_tiles` lists more tiles than the blur grid has workgroups and the blur
moves a pixel in every one of them, every blur case has a masked pixel that the blur changes (or is a declared identity), the
horizon case has W == 0 and both signs, the saturated frames reach both ends of the range.  No kernel runs here and no figure
comes from one; the tile constants come from the kernel's text, so an edit there that takes a case off its path fails here."""
import re

import numpy as np
import pytest

import warp_cases as wc

PATH_TAGS = ("ring", "no_ring", "wide", "outside", "lds", "bufend", "tiled", "one_bufend", "all_tiled", "lds_on_ring", "lds_inner",
             "whole_tile_inside")


def missing_path_tags(c, constants=None):
    """the entries of c.reach about tile paths that tile_paths does not confirm"""
    p = wc.tile_paths(c.M, *c.shape, c.dtype, constants)
    classes = list(p.tiles.values())
    lds = [k for k, v in p.tiles.items() if v == "lds"]
    have = {
        "ring": p.ring,
        "no_ring": not p.ring,
        "wide": p.gx >= 3 and p.gy < 3,
        "one_bufend": classes.count("bufend") == 1,
        "all_tiled": set(classes) == {"tiled"},
        "lds_on_ring": any(wc.on_ring(p, *k) for k in lds),
        "lds_inner": any(not wc.on_ring(p, *k) for k in lds),
        "whole_tile_inside": any(p.rows_xy[k] == 0 and p.rows_inside[k] > 0 for k in lds),
    }
    have.update({cls: cls in classes for cls in wc.TILE_CLASSES})
    return [t for t in c.reach if t in PATH_TAGS and not have[t]]


def test_constants_come_from_the_kernel_text():
    k = wc.CONSTANTS
    assert set(k) == {"WT_W", "TH_U8", "TH_U16", "LDS_DWORDS", "WT_SPLIT", "BT_H", "BT_W", "BLUR_GRID", "SCATTER_GRID"}
    assert all(v > 0 for v in k.values())
    with open(wc.KERNEL_TEXT) as f:
        text = f.read()
    with pytest.raises(RuntimeError, match="WT_SPLIT"):
        wc.read_constants(kernel_text=text.replace("constexpr int WT_SPLIT", "constexpr int WT_PARTS"))


def test_every_paths_case_reaches_the_path_in_its_name():
    for c in wc.cases_of("paths"):
        assert c.reach and all(t in PATH_TAGS for t in c.reach), wc.case_name(c)
        assert set(c.modes) == {0, 1, 2}
        for word in ("bufend", "lds", "tiled", "no_ring"):
            if c.name.startswith(word):
                assert ("all_tiled" if word == "tiled" else word) in c.reach, wc.case_name(c)
        assert missing_path_tags(c) == [], wc.case_name(c)
    for c in wc.CASES:      # the path entries of the other groups hold too
        if c.kind == "affine" and c.group != "paths":
            assert missing_path_tags(c) == [], wc.case_name(c)


def test_the_paths_table_reaches_every_class_on_ring_and_inner_tiles():
    for dt in wc.DTYPES:
        seen, rows_inside, rows_xy, grids = set(), 0, 0, set()
        for c in wc.cases_of("paths", dt):
            p = wc.tile_paths(c.M, *c.shape, c.dtype)
            grids.add(p.ring)
            seen |= {(cls, wc.on_ring(p, *k)) for k, cls in p.tiles.items()}
            rows_inside += sum(p.rows_inside.values())
            rows_xy += sum(p.rows_xy.values())
        name = np.dtype(dt).name
        assert seen == {(cls, ring) for cls in wc.TILE_CLASSES for ring in (False, True)}, (name, sorted(seen))
        assert rows_inside > 0 and rows_xy > 0, name
        assert grids == {False, True}, name
    shapes = {c.shape for c in wc.cases_of("paths")}
    k = wc.CONSTANTS
    assert any(h % k["TH_U8"] == 0 and w % k["WT_W"] == 0 for h, w in shapes), "a frame on the tile grid"
    assert any(h % k["TH_U8"] == 1 and w % k["WT_W"] == 0 for h, w in shapes), "a frame one row past the tile grid"
    p = wc.tile_paths(wc.IDENTITY, 96, 768, np.uint8)
    assert (p.gx, p.gy, p.ring) == (3, 3, True), "the smallest ring: one inner tile"


def test_a_retuned_tile_takes_cases_off_their_paths():
    """what the constants are read from the text for: with the LDS budget doubled the `lds` cases name themselves"""
    with open(wc.KERNEL_TEXT) as f:
        text = f.read()
    budget = wc.CONSTANTS["LDS_DWORDS"]
    edited, n = re.subn(r"(#define\s+MI_WARP_LDS_DWORDS\s+)\d+", lambda m: m.group(1) + str(2 * budget), text)
    assert n == 1
    k = wc.read_constants(kernel_text=edited)
    assert k["LDS_DWORDS"] == 2 * budget
    off = {c.name for c in wc.cases_of("paths") if missing_path_tags(c, k)}
    assert {"lds_scale_0.7_130x1030", "lds_shear_0.1_130x1030"} <= off, off
    assert not any(n_.startswith("bufend") for n_ in off), off


def test_blur_tiles_lists_the_tiles_with_a_masked_pixel():
    mask = np.ones((70, 130), np.uint8)
    assert wc.blur_tiles(mask) == set()
    mask[31, 63] = 0
    mask[32, 64] = 0
    mask[69, 129] = 0
    assert wc.blur_tiles(mask) == {(0, 0), (1, 1), (2, 2)}


def test_gauss_taps_sum_to_one():
    seen = set()
    for c in wc.CASES:
        for ks, sigma in c.blurs:
            key = (ks, sigma, np.dtype(c.dtype).itemsize * 8)
            if key in seen:
                continue
            seen.add(key)
            taps = wc.gauss_taps(ks, sigma, c.dtype)
            assert len(taps) == ks and int(taps.astype(np.int64).sum()) == 1 << key[2], key
            assert np.array_equal(taps, taps[::-1]), key
            identity = (ks, sigma) in wc.BLUR_IDENTITIES
            assert (np.count_nonzero(taps) == 1) == identity, (key, taps)
    assert {(k, s) for k, s, _b in seen} >= set(wc.BLURS) | set(wc.TINY_BLURS) | {wc.MANY_TILES_BLUR, wc.DEFAULT_BLUR}
    assert {b for _k, _s, b in seen} == {8, 16}


def masked_and_moved(c, ks, sigma):
    """(mask, which pixels the blur moved) of a mode-2 run"""
    plain, mask = wc.expected(c, 1)
    blurred, mask2 = wc.expected(c, 2, ks, sigma)
    assert np.array_equal(mask, mask2)
    moved = (plain != blurred).any(axis=2)
    assert not moved[mask != 0].any(), (wc.case_name(c), "the blur moved an in-frame pixel")
    return mask, moved


@pytest.mark.parametrize("group", ["blur", "tiny"])
def test_every_blur_case_has_a_masked_pixel_that_the_blur_moves(group):
    for c in wc.cases_of(group):
        name = wc.case_name(c)
        assert 2 in c.modes and ("masked" in c.reach) != ("blur_identity" in c.reach), name
        for ks, sigma in c.blurs:
            mask, moved = masked_and_moved(c, ks, sigma)
            assert (mask == 0).any(), (name, ks, sigma, "no masked pixel")
            if "blur_identity" in c.reach or c.shape == (1, 1):      # one tap, or one pixel: the blur of it is itself
                assert not moved.any(), (name, ks, sigma)
            else:
                assert moved.any(), (name, ks, sigma, "the blur moves nothing")
            if "unmasked" in c.reach:
                assert (mask != 0).any(), (name, "no unmasked pixel")
            if "all_masked" in c.reach:
                assert not mask.any(), (name, "an unmasked pixel")
    if group == "blur":
        assert {b for c in wc.cases_of("blur") for b in c.blurs} == set(wc.BLURS)
        largest = [c for c in wc.cases_of("blur") if "all_masked" in c.reach]
        assert {c.dtype for c in largest} == set(wc.DTYPES) and all(c.blurs == ((31, 50.0),) and c.name.startswith(wc.ALL_MASKED)
                                                                    for c in largest)
    else:
        assert {c.shape for c in wc.cases_of("tiny")} == set(wc.TINY_SHAPES)
        assert any(min(c.shape) < ks // 2 for c in wc.cases_of("tiny") for ks, _s in c.blurs), "a frame below the blur radius"


def test_many_tiles_lists_more_tiles_than_the_blur_grid():
    k = wc.CONSTANTS
    cases = wc.cases_of("many_tiles")
    assert {(c.kind, c.dtype) for c in cases} == {(kind, dt) for kind in ("affine", "perspective") for dt in wc.DTYPES}
    for c in cases:
        name = wc.case_name(c)
        (ks, sigma), = c.blurs
        mask, moved = masked_and_moved(c, ks, sigma)
        tiles = wc.blur_tiles(mask)
        assert len(tiles) > max(k["BLUR_GRID"], k["SCATTER_GRID"]), (name, len(tiles))
        moved_tiles = wc.blur_tiles(~moved)
        assert moved_tiles == tiles, (name, "tiles the blur leaves as they are", sorted(tiles - moved_tiles)[:5])
    a, b = (wc.expected(c, 2, *wc.MANY_TILES_BLUR) for c in cases if c.dtype == np.uint16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the 3 x 3 form of the shift is the same warp"


def test_transform_cases_do_what_they_are_there_for():
    for c in wc.cases_of("transforms") + wc.cases_of("perspective"):
        name = wc.case_name(c)
        img = wc.frame_of(c)
        out, mask = wc.expected(c, 1)
        if "first_pixel" in c.reach:        # the inverse of a singular matrix is all zeros: every pixel reads source (0, 0)
            assert mask.all() and (out == img[0, 0]).all(), name
        if "all_masked" in c.reach:
            assert not mask.any(), name
        if "mixes_border" in c.reach:       # in frame, and the constant border enters the value
            mixed = wc.expected(c, 0)[0]
            border = np.array(wc.border_value(c.dtype)[:3], c.dtype)
            assert mask.all() and (mixed != img).all() and (mixed != border).all(), name
        if "mask_tie" in c.reach:
            # half a pixel out of frame is an in-image weight of exactly 16384 of 32768: (16384 + 16384) >> 15 = 1, in frame;
            # a quarter (the corner under (0.5, 0.5)) is 8192: masked
            dx, dy = c.M[0][2], c.M[1][2]
            assert int((mask == 0).sum()) == (1 if dx and dy else 0), name
            if c.dtype == np.uint16 and dy == 0:
                a, b = img[:, :-1].astype(np.int64), img[:, 1:].astype(np.int64)
                ties = ((a + b) & 1) == 1
                assert ties.mean() > 0.25, name
                half_even = (a + b) // 2 + (((a + b) & 1) & ((a + b) // 2 & 1))
                assert np.array_equal(out[:, 1:], half_even), (name, "rintf rounds the .5 sums to even")
    names = {c.name for c in wc.cases_of("transforms")}
    assert {"rotation_180", "mirror_x", "rotation_90_300x300", "zoom_out_2x_200x800", "singular_9x11", "singular_70x777",
            "shift_1e5"} <= names
    # 180 degrees and the mirror, away from the half-pixel of rounding, are flips of the frame
    for c in wc.cases_of("transforms"):
        if c.name == "mirror_x":
            out, mask = wc.expected(c, 1)
            assert mask.all() and np.array_equal(out, wc.frame_of(c)[:, ::-1]), wc.case_name(c)


def test_perspective_table_has_the_block_edges_and_the_horizon():
    shapes = set(wc.PERSPECTIVE_SHAPES)
    bw0 = {(h, w): min(1024 // min(16, h), w) for h, w in shapes}
    assert bw0[(5, 300)] == 204 and bw0[(1, 1100)] == 1024
    assert any(h < 16 and w > bw0[(h, w)] for h, w in shapes)
    assert any(w == bw0[(h, w)] for h, w in shapes), "w <= bw0: one block"
    assert any(w > bw0[(h, w)] and w % bw0[(h, w)] == 0 for h, w in shapes), "w a multiple of bw0"
    assert any(w % bw0[(h, w)] not in (0, w) for h, w in shapes), "a last block that ends early"
    for dt in wc.DTYPES:
        have = {(c.shape, c.name.split("_")[0]) for c in wc.cases_of("perspective", dt)}
        assert have >= {(s, n) for s in shapes for n in ("mild", "strong", "singular")}
        horizon, = [c for c in wc.cases_of("perspective", dt) if "horizon" in c.reach]
        assert wc._oracle_invert_3x3(horizon.M) == [float(v) for row in horizon.M for v in row], "its own inverse, exactly"
        W = wc.perspective_w(horizon)
        assert (W == 0).any() and (W < 0).any() and (W > 0).any()
        assert np.array_equal(np.nonzero((W == 0).any(axis=0))[0], [64])
        out, mask = wc.expected(horizon, 1)
        assert (out[:, 64] == wc.frame_of(horizon)[0, 0]).all() and mask[:, 64].all(), "W == 0 reads source (0, 0)"
        assert (mask == 0).any() and (mask != 0).any()


def test_values_cases_reach_both_ends_of_the_range():
    for c in wc.cases_of("values"):
        vmax = wc.vmax_of(c.dtype)
        assert set(c.reach) <= {"has_max", "has_zero"} and c.reach
        for mode, ks, sigma in wc.runs_of(c):
            out, _mask = wc.expected(c, mode, ks, sigma)
            if "has_max" in c.reach:
                assert (out == vmax).any(), (wc.case_name(c), mode)
            if "has_zero" in c.reach:
                assert (out == 0).any(), (wc.case_name(c), mode)
    assert {c.frame for c in wc.cases_of("values")} == {"max", "zero", "checker", "columns"}


def test_the_table_stays_small():
    for c in wc.CASES:
        h, w = c.shape
        assert h * w < (1 << 20) or c.group == "many_tiles", wc.case_name(c)
        assert wc.runs_of(c), wc.case_name(c)


def test_device_and_scratch_inputs_reach_what_they_are_there_for():
    h, w = wc.DEVICE_SHAPE
    assert w % 4 == 0
    (_zoom, staged), (_shift, per_pixel) = wc.DEVICE_TRANSFORMS
    for dt in wc.DTYPES:
        assert set(wc.tile_paths(staged, h, w, dt).tiles.values()) == {"tiled"}
        p = wc.tile_paths(per_pixel, h, w, dt)
        assert "outside" in p.tiles.values() and sum(p.rows_inside.values()) > 0 and sum(p.rows_xy.values()) > 0
        for kind in ("affine", "perspective"):
            M = np.array(per_pixel if kind == "affine" else wc.as_3x3(per_pixel), np.float64)
            img = wc.device_frame(dt)
            plain, mask = wc.oracle_warp(kind, img, M, 1)
            blurred, _mask = wc.oracle_warp(kind, img, M, 2, *wc.DEVICE_BLUR)
            assert (mask == 0).any() and (mask != 0).any() and (plain != blurred).any()
        seq = wc.scratch_sequence(dt)
        sizes = [img.shape[0] * img.shape[1] for _k, img, *_rest in seq]
        assert sizes[2] > sizes[0] > sizes[4] and sizes[6] == sizes[0], "large after small, small after large, the first again"
        for kind, img, M, ks, sigma in seq:
            _out, mask = wc.oracle_warp(kind, img, M, 2, ks, sigma)
            assert (mask == 0).any()
