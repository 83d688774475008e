"""CPU: the cases of tests/depth_smooth_cases.py, stereo_cases.py, composite_cases.py and brush_cases.py, checked from the NumPy
restatements so that the GPU sweep over them (test_gpu_depth_outputs_edges.py) cannot pass on inputs that say nothing.
Everything asserted here is a condition on the inputs: every path label of a kernel occurs among its cases, every "mixed" plane
has both outcomes, the samples that are compared NaN-aware (where the restatement's own output is a NaN it computed) stay under
1 % of every case, and no GPU case exceeds 1025 x 70 pixels.  No kernel runs here and no figure comes from one."""
import numpy as np
import pytest

import brush_cases as bc
import brush_restatement as br
import composite_cases as cc
import depth_render_restatement as drr
import depth_restatement as dr
import depth_smooth_cases as sc
import stereo_cases as vc
import stereo_restatement as sr

MAX_PIXELS = 1025 * 70
NAN_SHARE = 0.01


# ---------------------------------------------------------------- smoothing
def test_smoothing_table_reaches_the_segment_and_workgroup_edges():
    shapes = {c.shape: c for c in sc.TABLE}
    for c in sc.TABLE:
        assert c.radius == dr.radius_of(c.sigma) < min(c.shape), sc.case_name(c)
        assert c.shape[0] * c.shape[1] <= MAX_PIXELS
    # two row segments with the widest halo, which the height allows exactly: radius == h - 1
    for w in (sc.SEG - 1, sc.SEG, sc.SEG + 1, sc.SEG + 48, sc.SEG + 49):
        assert shapes[(49, w)].radius == 48 == 49 - 1
    assert shapes[(70, 49)].radius == 49 - 1                            # the radius at the width's limit
    for h in (sc.COL_ROWS - 1, sc.COL_ROWS, sc.COL_ROWS + 1):
        assert shapes[(h, 70)].radius == 30                             # 30 is the largest radius 3 sigma gives below 31
    for h in (2 * sc.COL_ROWS - 1, 2 * sc.COL_ROWS, 2 * sc.COL_ROWS + 1):
        assert shapes[(h, 70)].radius == 48
    assert shapes[(5, 2 * sc.SEG + 1)].radius == 2                      # a last segment of one pixel
    assert set(sc.WORK_TYPES) == {np.float32, np.float64} and len(sc.runs()) == len(sc.TABLE) * 2 * 2 * 3


@pytest.mark.parametrize("work", sc.WORK_TYPES, ids=lambda d: np.dtype(d).name)
def test_smoothing_weight_planes_have_both_outcomes(work):
    seen_nan_output = 0
    for c in sc.TABLE:
        name = (sc.case_name(c), np.dtype(work).name)
        den = sc.blurred_weight(c, "mixed", work)
        assert np.isfinite(den).all() and (den > 0).mean() >= 0.1 and (den <= 0).mean() >= 0.1, name
        assert (sc.blurred_weight(c, "positive", work) > 0).all(), name
        wt = sc.weight_plane(c.shape, c.radius, "special", work)
        sites = sc.special_sites(c.shape, c.radius)
        assert len(set(sites.values())) == len(sites) == 5
        assert all(wt[at] == 0 and np.signbit(wt[at]) for k, at in sites.items() if k.startswith("-0"))
        assert np.isnan(wt[sites["nan"]]) and wt[sites["inf"]] == np.inf and np.isfinite(wt).sum() == wt.size - 2
        den = sc.blurred_weight(c, "special", work)
        assert np.isnan(den).any() and (den > 0).any(), name            # the fallback to v beside pixels that divide
        for vk in sc.VALUE_KINDS:
            v = sc.value_plane(c.shape, vk, work)
            assert v.dtype == (np.int32 if vk == "int32" else work)
            for wk in sc.WEIGHT_KINDS:
                want = sc.expected(c, vk, wk, work)
                share = float(np.isnan(want).mean())
                assert share < NAN_SHARE, (name, vk, wk, share)
                if wk != "special":
                    assert share == 0.0, (name, vk, wk)
                seen_nan_output += int(np.isnan(want).sum())
                # where B(w) is not positive the output is the value itself
                fallback = ~(sc.blurred_weight(c, wk, work) > 0)
                assert np.array_equal(want[fallback], np.asarray(v)[fallback].astype(np.float32)), (name, vk, wk)
                assert not np.array_equal(want, np.asarray(v).astype(np.float32)), (name, vk, wk)
    assert seen_nan_output > 0      # the +inf weights do give NaN outputs: the NaN-aware compare is exercised


def test_smoothing_max_map_frames():
    frames = sc.max_map_frames()
    h, w = sc.MAX_MAP_SHAPE
    assert len(frames) >= 3 and w > sc.SEG and all(f.shape == (h, w, 3) and f.dtype == np.uint8 for f in frames)
    assert all(dr.radius_of(s) < min(h, w) for s in sc.MAX_MAP_SIGMAS) and dr.radius_of(max(sc.MAX_MAP_SIGMAS)) == 48
    assert h * w <= MAX_PIXELS


# ---------------------------------------------------------------- stereo
def test_stereo_cases_cover_the_table():
    seen = {(c.width, c.kind, c.shift, c.pivot, c.near) for c in vc.VIEW_CASES}
    for w in (65, 511, 512, 513, 1024, 1025):
        for kind in ("steps", "random", "ramp", "special"):
            assert seen >= {(w, kind, s, p, n) for s in (64.0, -64.0) for p in (0.0, 0.3, 1.0) for n in ("last", "first")}
        assert vc.ROWS * w <= MAX_PIXELS
    assert np.ceil(64.0) == 65 - 1
    w, s = vc.NARROW
    assert np.ceil(s) == w - 1 and s != int(s) and any(c.width == w and c.shift == -s for c in vc.VIEW_CASES)
    for w in vc.WIDTHS:
        z = vc.plane("special", w)
        assert np.isnan(z).any() and (z == np.inf).any() and (z == -np.inf).any() and ((z == 0) & np.signbit(z)).any()
        for kind in ("steps", "random", "ramp"):
            assert np.isfinite(vc.plane(kind, w)).all()
    assert vc.GROUPS == sorted(set(vc.WIDTHS) | {vc.NARROW[0]} | {w for w, _ in vc.EMPTY_ROWS})


def test_stereo_predictor_agrees_with_the_restatement_and_every_label_occurs():
    seen = {}
    for c in vc.VIEW_CASES:
        for lb in vc.labels(c):
            seen.setdefault(lb, []).append(c)
        xs = vc.source_map(c)
        assert xs.shape == (vc.ROWS, c.width) and xs.min() >= 0 and xs.max() < c.width
        assert np.abs(xs - np.arange(c.width)).max() <= 2 * 64 + 2
    assert set(seen) == set(vc.LABELS), set(vc.LABELS) - set(seen)
    # the source map is sr.view's
    for c in vc.VIEW_CASES[::37] + [c for c in vc.VIEW_CASES if c.kind == "halves"]:
        for dt in vc.DTYPES:
            img = vc.image((vc.ROWS, c.width), dt)
            assert np.array_equal(vc.expected_view(c, dt), sr.view(img, vc.plane(c.kind, c.width), vc.N_FRAMES, c.shift, c.pivot, c.near))
    # what the `steps` plane reaches: 64-wide holes and sources that cross a segment boundary from 513 on, none at 511 and 512
    for w in vc.WIDTHS:
        steps = [c for c in vc.VIEW_CASES if c.width == w and c.kind == "steps"]
        crossing = any("source into another segment" in vc.labels(c) for c in vc.VIEW_CASES if c.width == w)
        assert crossing == (w > vc.SEG), w
        if w > vc.SEG:
            assert any("hole of 64" in vc.labels(c) for c in steps), w
            assert any("source into another segment" in vc.labels(c) for c in steps), w
            assert any("hole neighbour in another segment" in vc.labels(c) for c in steps), w
    # the planes with NaN, infinities and -0 reach occlusions and holes on their own
    special = set().union(*(vc.labels(c) for c in vc.VIEW_CASES if c.kind == "special"))
    assert special >= {"occluded", "hole from the left", "hole from the right", "hole with one side"}
    # the narrow row: both ends of the displacement range are reached
    for c in vc.VIEW_CASES:
        if c.width == vc.NARROW[0] and c.kind != "halves":
            assert vc.labels(c) & {"occluded", "hole from the left", "hole from the right", "hole with one side"}, vc.view_name(c)


def test_stereo_rows_that_no_source_lands_on():
    """rint rounds both half-way ends of the displacement outward: at pivot 0.5 and an odd shift s = W - 1, which the checks
    accept (ceil(|shift|) < W), the two ends are (s + 1) / 2 either way, W apart.  Every case of the `halves` plane has rows
    that lose every source over the edges -- their targets keep their own pixels -- next to rows where every source lands and
    a row that a single source enters or leaves differently; both signs of the shift, both `near`, three widths"""
    from shinestacker_amd import stereo
    cases = [c for c in vc.VIEW_CASES if c.kind == "halves"]
    assert {(c.width, c.shift, c.near) for c in cases} == {(w, sg * s, n) for w, s in vc.EMPTY_ROWS for sg in (1, -1) for n in vc.NEARS}
    for c in cases:
        assert stereo.check_shift(c.shift, c.width) == c.shift and c.pivot == 0.5 and abs(c.shift) == c.width - 1
        a, b = vc.displacement_span(vc.N_FRAMES, c.shift, c.pivot)
        assert a == b == c.width // 2 and a + b == c.width
        assert vc.NO_SIDE in vc.labels(c) and len(vc.labels(c)) >= 2, vc.view_name(c)     # and a row with a hole that has a side
        z, xs = vc.plane(c.kind, c.width), vc.source_map(c)
        empty = [y for y in range(vc.ROWS) if vc.row_labels(z[y], vc.N_FRAMES, c.shift, c.pivot, c.near) == {vc.NO_SIDE}]
        full = [y for y in range(vc.ROWS) if not vc.row_labels(z[y], vc.N_FRAMES, c.shift, c.pivot, c.near)]
        assert len(empty) >= 2 and len(full) >= 2 and len(empty) + len(full) == vc.ROWS - 1, vc.view_name(c)
        for y in empty:
            assert np.array_equal(xs[y], np.arange(c.width))
        for y in full:      # the two halves change places
            assert np.array_equal(xs[y], (np.arange(c.width) + c.width // 2) % c.width)
    assert not any(vc.NO_SIDE in vc.labels(c) for c in vc.VIEW_CASES if c.kind != "halves")


def test_stereo_device_and_anaglyph_cases():
    u8 = {(s, o) for dt, s, o in vc.DEVICE_CASES if dt == np.uint8}
    u16 = {(s, o) for dt, s, o in vc.DEVICE_CASES if dt == np.uint16}
    assert {o for _, o in u8} == {0, 1, 2, 3} and {s for s, _ in u8} == {0, 1, 2, 3}
    assert (2, 0) in u16 and {o for _, o in u16} == {0, 2}               # a uint16 frame at a 2-byte-odd address
    c = vc.DEVICE_VIEW
    assert c.width % 4 == 1 and vc.labels(c) >= {"hole of 64", "source into another segment", "occluded"}
    tails = {dt: [vc.tail_samples(s, dt) for s in vc.ANAGLYPH_SHAPES] for dt in vc.DTYPES}
    assert tails == {np.uint8: [3, 2, 1], np.uint16: [1, 0, 1]}
    assert {t for v in tails.values() for t in v} == {0, 1, 2, 3}


# ---------------------------------------------------------------- composite
def composite_runs():
    """(shape, n, run) of the GPU file's table"""
    return [(s, cc.N_SHORT, r) for s in cc.SHAPES for r in ("whole", "chunks")] + [(cc.LONG_SHAPE, cc.N_LONG, "whole")]


def test_composite_launches_and_sizes():
    assert cc.launches(0, cc.N_LONG) == [(0, 64), (63, 64), (126, 2)]       # a third launch of exactly 2
    assert cc.launches(0, 5) == [(0, 5)] and cc.launches(2, 3) == [(2, 3)] and cc.launches(0, 65) == [(0, 64), (63, 2)]
    assert cc.calls_of("chunks", cc.N_SHORT) == [(0, 3), (2, 3)]
    assert sorted(h * w for h, w in cc.SHAPES) == [1, 5, 1023, 1024, 1025]
    assert cc.LONG_SHAPE in cc.SHAPES and max(h * w for h, w in cc.SHAPES) <= MAX_PIXELS


def composite_layouts(dtype):
    """(shape, n, run, layout) of the GPU file's runs for one dtype: the frames of the short stack in allocations of their own,
    the long stack in slots of one allocation, and for uint16 the short stack 2 bytes off the 4-byte boundaries"""
    out = [(s, n, r, "separate" if n == cc.N_SHORT else "slots") for s, n, r in composite_runs()]
    if dtype == np.uint16:
        out += [(cc.LONG_SHAPE, cc.N_SHORT, r, lay) for lay in ("off 1", "off 2") for r in ("whole", "chunks")]
    return out


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.dtype_name)
def test_composite_every_path_occurs(dtype):
    """the share of the written pixels on each path, over every launch of every run, from the planes and from where the
    dtype's frames lie"""
    for interp in cc.INTERPS:
        total, by_run = {}, {}
        for shape, n, run, layout in composite_layouts(dtype):
            offsets = cc.frame_offsets(shape, n, dtype, layout)
            assert len(offsets) == n and all(o % np.dtype(dtype).itemsize == 0 for o in offsets)
            for kind in cc.PLANES:
                z = cc.plane(kind, shape, n)
                assert z.shape == shape and z.dtype == np.float32
                for first, count in cc.calls_of(run, n):
                    for f0, c in cc.launches(first, count):
                        part = cc.wave_paths(z, n, f0, c, interp == "nearest", offsets)
                        cc.add(total if layout in ("separate", "slots") else {}, part)
                        cc.add(by_run.setdefault((shape, n, run, layout), {}), part)
        written = sum(total.values())
        share = {k: total[k] / written for k in cc.PATHS}
        assert all(s >= 0.02 for s in share.values()), (cc.dtype_name(dtype), interp, share)
        assert total[cc.UNALIGNED] == 0         # slots of a 4-byte multiple keep every frame of every dtype aligned
        # the chunk boundary exists only where a call does not hold the whole stack, or spans more than one launch
        for (shape, n, run, layout), part in by_run.items():
            if run == "whole" and n <= cc.TAB:
                assert part["gather: chunk boundary"] == 0
            elif shape[0] * shape[1] > 1000:
                assert part["gather: chunk boundary"] > 0, (shape, n, run)
        # the frame's end: in a lane at 1023 and 1025 pixels, on a wave's last lane at 1024
        for shape in cc.SHAPES:
            ends = by_run[(shape, cc.N_SHORT, "whole", "separate")]["gather: frame end"]
            assert (ends > 0) == (shape[0] * shape[1] % cc.LANE_PX != 0), shape
        if dtype == np.uint16:
            # every frame off the boundary: no wave is fast; every second frame: the waves that read only frames 1 and 3 still are
            for run in ("whole", "chunks"):
                every, second = by_run[(cc.LONG_SHAPE, cc.N_SHORT, run, "off 1")], by_run[(cc.LONG_SHAPE, cc.N_SHORT, run, "off 2")]
                aligned = by_run[(cc.LONG_SHAPE, cc.N_SHORT, run, "separate")]
                assert every["fast"] == 0 and every[cc.UNALIGNED] == aligned["fast"] > 0, (run, interp, every)
                assert second[cc.UNALIGNED] > 0 and second["fast"] + second[cc.UNALIGNED] == aligned["fast"], (run, interp, second)
            assert any(by_run[(cc.LONG_SHAPE, cc.N_SHORT, run, "off 2")]["fast"] > 0 for run in ("whole", "chunks")) or interp == "linear"
    assert [o % 4 for o in cc.frame_offsets(cc.LONG_SHAPE, 5, np.uint16, "off 1")] == [2] * 5
    assert [o % 4 for o in cc.frame_offsets(cc.LONG_SHAPE, 5, np.uint16, "off 2")] == [2, 0, 2, 0, 2]
    assert all(o % 4 == 0 for dt in cc.DTYPES for o in cc.frame_offsets(cc.LONG_SHAPE, cc.N_LONG, dt, "slots"))
    assert cc.frame_offsets(cc.LONG_SHAPE, 3, np.uint8, "slots")[1] == 3076      # 3075 bytes a frame: packed, every second one would be off


def test_composite_float32_frames_carry_the_special_values():
    sp = cc.specials()
    assert sp.view(np.uint32).tolist() == [0x80000000, 0x7F800000, 0xFF800000, cc.NAN_PAYLOAD] and np.isnan(sp[3])
    for shape, n, _ in composite_runs():
        frames = cc.frames(shape, n, np.float32)
        bits = np.stack(frames).view(np.uint32)
        held = [b for b in sp.view(np.uint32) if shape != (1, 1) or b != 0xFF800000]      # three samples hold three of the four
        for b in held:
            assert (bits == b).any(), (shape, n, hex(int(b)))
        assert np.isfinite(np.stack(frames)).mean() > 0.98 or shape[0] * shape[1] < 100       # next to finite samples
        # integer depths select them: each special value is in the expected output, byte for byte, for both interp
        for interp in cc.INTERPS:
            want = cc.expected(shape, n, np.float32, "integer", interp)
            z = cc.plane("integer", shape, n)
            assert np.array_equal(z, np.rint(z)) and not cc.computed_nan(want, z, n, interp).any()
            pick = np.take_along_axis(np.stack(frames), drr.indices(z, n)[4][None, :, :, None], 0)[0]
            assert want.tobytes() == pick.tobytes()
            for b in held:
                assert (want.view(np.uint32) == b).any(), (shape, n, interp, hex(int(b)))
    for dt in (np.uint8, np.uint16):
        assert all(f.dtype == dt for f in cc.frames((1, 5), 5, dt))


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.dtype_name)
def test_composite_nan_aware_samples_stay_under_one_per_cent(dtype):
    some = 0
    for shape, n, _ in composite_runs():
        for kind in cc.PLANES:
            z = cc.plane(kind, shape, n)
            for interp in cc.INTERPS:
                want = cc.expected(shape, n, dtype, kind, interp)
                computed = cc.computed_nan(want, z, n, interp)
                assert computed.mean() < NAN_SHARE, (shape, n, kind, interp, float(computed.mean()))
                some += int(computed.sum())
                if kind == "fractional":
                    f = drr.indices(z, n)[2]
                    assert 0.02 <= (f == 0).mean() or z.size < 100
                    assert (f != 0).mean() >= 0.5
    assert (some > 0) == (dtype == np.float32)


# ---------------------------------------------------------------- brush
def test_brush_one_tile_hit_counts_sit_on_the_chunk_limits():
    size, _, _, flow = bc.ONE_TILE_BRUSH
    radius = br.radius_of(size)
    assert radius <= bc.MAX_RADIUS and radius >= bc.TW - 1 and flow == 7
    assert set(bc.HIT_COUNTS) == {255, 256, 257, 511, 512, 513, 769}
    for n in bc.HIT_COUNTS:
        stamps = br.centres(bc.one_tile_points(n))
        hits = bc.tile_hits(stamps, radius, bc.ONE_TILE_SHAPE)
        assert hits.shape[:2] == (1, 1) and hits.sum() == n == len(stamps)      # one tile, every stamp hits it
        for cx, cy in stamps:
            assert br.footprint(cx, cy, radius, *bc.ONE_TILE_SHAPE) == (0, 0, bc.TW, bc.TH)
        _, layer, _ = bc.expected(bc.ONE_TILE_SHAPE, np.uint16, bc.one_tile_points(n), bc.ONE_TILE_BRUSH)
        assert 0 < layer.min() and layer.max() < 1
        other = br.stroke_fold(*bc.frames(bc.ONE_TILE_SHAPE, np.uint16), bc.table_of(bc.ONE_TILE_BRUSH),
                               br.centres(bc.shuffled(bc.one_tile_points(n))), radius, bc.ONE_TILE_BRUSH[2], flow)[1]
        assert not np.array_equal(other, layer), n


def test_brush_ragged_stroke_shares_its_blocks_among_the_tiles():
    size, _, opacity, flow = bc.RAGGED_BRUSH
    radius = br.radius_of(size)
    pts = bc.ragged_points()
    stamps = br.centres(pts)
    h, w = bc.RAGGED_SHAPE
    assert len(stamps) >= 800 and radius <= bc.MAX_RADIUS and flow == 7 and h * w <= MAX_PIXELS
    hits = bc.tile_hits(stamps, radius, bc.RAGGED_SHAPE)
    ny, nx, nb, nw = hits.shape
    assert ny >= 3 and nx >= 3 and nb >= 4 and nw == 4
    per_block = hits.sum(axis=3)
    assert per_block.sum(axis=2).min() > 0                              # the walk meets every tile of its box
    ragged = ((per_block >= 1) & (per_block <= 255)).sum(axis=2)
    assert ragged.max() >= 3, ragged                                    # a tile with a ragged share of at least three blocks
    assert (ragged >= 3).sum() >= 4
    assert ((hits == 0) & (per_block[..., None] > 0)).any()             # a wave without a hit inside a block that has some
    assert ((hits > 0) & (hits < bc.WAVE)).any()                        # and waves that hit in part: the ballot's rank matters
    # the stamp list outruns the frame a little: a stamp outside the frame pulls the undo area to the origin
    _, layer, area = bc.expected(bc.RAGGED_SHAPE, np.uint16, pts, bc.RAGGED_BRUSH)
    assert area[:2] == (0, 0) and 0 < layer.max() < 1 and (layer > 0).mean() > 0.5
    other = br.stroke_fold(*bc.frames(bc.RAGGED_SHAPE, np.uint16), bc.table_of(bc.RAGGED_BRUSH), br.centres(bc.shuffled(pts)), radius,
                           opacity, flow)[1]
    assert not np.array_equal(other, layer)
    for dt in bc.DTYPES:
        out = bc.expected(bc.RAGGED_SHAPE, dt, pts, bc.RAGGED_BRUSH)[0]
        assert (out != bc.frames(bc.RAGGED_SHAPE, dt)[0]).mean() > 0.05
