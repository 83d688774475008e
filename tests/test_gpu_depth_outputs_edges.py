"""GPU: what the stackers make of the depth map -- the weighted smoothing (csrc/kernels_depth.hpp), the stereo view and the
anaglyph (kernels_stereo.hpp), the depth-selected composite (kernels_composite.hpp) and the brush stroke (kernels_brush.hpp) --
against their NumPy restatements on the cases of tests/depth_smooth_cases.py, stereo_cases.py, composite_cases.py and
brush_cases.py: rows of two and three 256-pixel segments with a 48-pixel halo, heights next to the column pass's workgroups,
mixed-sign, -0, infinite and NaN weights, the unweighted smoothing of DepthMapStack's MAX map; views at widths next to the
512-target segment, shifts as wide as the row, rows that no source lands on, NaN and infinite depths, frames and outputs on every byte phase with guard bytes
around them, anaglyphs with 0 to 3 tail samples; float32 composites of -0, infinities and a NaN with a payload, frames that end
inside a lane, unaligned uint16 frames, 128 frames in three launches; strokes whose hit counts sit on the limits of the ordered
compaction.  Every comparison is array_equal or byte equality; a NaN that the restatement itself computed is compared as a NaN
(the sign bit of a generated NaN differs between x86 and gfx950).  test_depth_outputs_cases_host.py checks on the CPU that
the cases reach every path and that such samples stay under 1 % of every case."""

import numpy as np
import pytest

import brush_cases as bc
import composite_cases as cc
import depth_restatement as dr
import depth_smooth_cases as sc
import stereo_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


def freed(buffers):
    for b in buffers:
        b.free()


# ---------------------------------------------------------------- smoothing
@pytest.mark.parametrize("case", sc.TABLE, ids=sc.case_name)
def test_weighted_smooth_equals_the_restatement(dev, case):
    from shinestacker_amd import depth_out
    for c, vk, wk, work in sc.runs():
        if c != case:
            continue
        name = (sc.case_name(c), vk, wk, np.dtype(work).name)
        v, w = sc.value_plane(c.shape, vk, work), sc.weight_plane(c.shape, c.radius, wk, work)
        got = depth_out.weighted_smooth(v, w, c.sigma)
        want = sc.expected(c, vk, wk, work)
        if np.isnan(want).any():
            assert wk == "special", name
            assert sc.same_but_nan(got, want), (name, int((got != want).sum()))
        else:
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (name, int((got != want).sum()),
                                                                                np.argwhere(got != want)[:5])


def test_unweighted_smoothing_of_the_max_map(dev):
    """w == nullptr in ws_rows: DepthMapStack(map_type='max') smooths its depth map with every weight 1"""
    from shinestacker_amd import DepthMapStack
    frames = list(sc.max_map_frames())
    dms = DepthMapStack(map_type="max")
    try:
        dms.focus_stack_arrays(frames)
        h = dms._dmap
        ins = np.stack([h.tap(dev.DM_TAP_ENERGY_IN, i) for i in range(len(frames))])
        tot = h.tap(dev.DM_TAP_TOTAL)
        plain = dms.depth_map(0.0)
        assert np.array_equal(plain, dr.depth_map_stack(ins, tot, 0.0, False)) and plain.max() > plain.min()
        for sigma in sc.MAX_MAP_SIGMAS:
            got = dms.depth_map(sigma)
            want = dr.depth_map_stack(ins, tot, sigma, False)
            assert got.dtype == np.float32 and got.shape == sc.MAX_MAP_SHAPE
            assert np.array_equal(got, want), (sigma, int((got != want).sum()))
            assert not np.array_equal(got, plain)
    finally:
        dms.close()


# ---------------------------------------------------------------- stereo
@pytest.mark.parametrize("width", vc.GROUPS)
def test_view_equals_the_restatement(dev, width):
    from shinestacker_amd import stereo
    cases = [c for c in vc.VIEW_CASES if c.width == width]
    assert cases
    for c in cases:
        z = vc.plane(c.kind, c.width)
        for dtype in vc.DTYPES:
            img = vc.image((vc.ROWS, c.width), dtype)
            got = stereo.view(img, z, vc.N_FRAMES, c.shift, c.pivot, c.near)
            want = vc.expected_view(c, dtype)
            assert got.dtype == want.dtype and np.array_equal(got, want), (vc.view_name(c), np.dtype(dtype).name,
                                                                         np.argwhere((got != want).any(axis=2))[:5])


@pytest.mark.parametrize("dtype,src_off,out_off", vc.DEVICE_CASES)
def test_view_device_on_every_byte_phase_leaves_the_guard_bytes(dev, dtype, src_off, out_off):
    from shinestacker_amd import stereo
    c = vc.DEVICE_VIEW
    shape = (vc.ROWS, c.width)
    img, z = vc.image(shape, dtype), vc.plane(c.kind, c.width)
    want = vc.expected_view(c, dtype)
    fb = img.nbytes
    lead = vc.GUARD + out_off           # the output starts `out_off` bytes after a 4-byte boundary
    assert vc.GUARD % 4 == 0
    guard = np.random.default_rng(src_off * 4 + out_off).integers(0, 256, lead + fb + vc.GUARD).astype(np.uint8)
    bufs = []
    try:
        for nbytes in (fb + 4, z.nbytes, guard.nbytes):
            bufs.append(dev.DeviceBuffer(nbytes))
        src, dep, out = bufs
        src.upload(img, src_off)
        dep.upload(z)
        out.upload(guard)
        stereo.view_device(src.ptr + src_off, dep.ptr, out.ptr + lead, shape[0], shape[1], dtype, vc.N_FRAMES, c.shift, c.pivot, c.near)
        dev.check(dev.load().mi_device_synchronize(0))
        back = out.download(guard.shape, np.uint8)
        assert back[lead:lead + fb].tobytes() == want.tobytes()
        assert np.array_equal(back[:lead], guard[:lead]) and np.array_equal(back[lead + fb:], guard[lead + fb:])
        assert np.array_equal(src.download(img.shape, dtype, src_off), img)
    finally:
        freed(bufs)


@pytest.mark.parametrize("dtype", vc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_anaglyph_tails(dev, dtype):
    """0 to 3 samples after the last whole word: the kernel on two unrelated frames, and stereo.pair where a row takes a shift"""
    from shinestacker_amd import stereo
    import stereo_restatement as sr
    for shape in vc.ANAGLYPH_SHAPES:
        h, w = shape
        left, right = vc.image(shape, dtype, 11), vc.image(shape, dtype, 12)
        want = stereo.compose(left, right, "anaglyph")
        fill = np.full(left.nbytes + 8, 0x5A, np.uint8)
        bufs = []
        try:
            for _ in range(3):
                bufs.append(dev.DeviceBuffer(left.nbytes + 8))
            bufs[0].upload(left)
            bufs[1].upload(right)
            bufs[2].upload(fill)
            dev.check(dev.load().mi_stereo_compose_device(0, None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, h, w, dev.DTYPE_CODE[np.dtype(dtype)],
                                                          stereo.LAYOUTS["anaglyph"]))
            dev.check(dev.load().mi_device_synchronize(0))
            back = bufs[2].download(fill.shape, np.uint8)
            assert back[:left.nbytes].tobytes() == want.tobytes(), (shape, vc.tail_samples(shape, dtype))
            assert np.array_equal(back[left.nbytes:], fill[left.nbytes:]), shape
        finally:
            freed(bufs)
        if w > 1:       # a separation needs a row of two pixels: a single pixel only takes the shift 0
            z = np.linspace(0.0, vc.N_FRAMES - 1, h * w, dtype=np.float32).reshape(shape)
            got = stereo.pair(left, z, vc.N_FRAMES, 2.0, 0.5, "last", "anaglyph")
            assert np.array_equal(got, sr.pair(left, z, vc.N_FRAMES, 2.0, 0.5, "last", "anaglyph")), shape
        else:
            assert np.array_equal(stereo.view(left, np.zeros(shape, np.float32), vc.N_FRAMES, 0.0), left)


# ---------------------------------------------------------------- composite
def composite_run(dev, frames_dev, shape, n, dtype, run):
    """every plane and both interp over frames already on the device, rendered whole or in chunks into a prefilled output"""
    from shinestacker_amd import depth_render
    h, w = shape
    fb = h * w * 3 * np.dtype(dtype).itemsize
    fill = np.full(shape + (3,), cc.SENTINEL[dtype], dtype)
    bufs = []
    try:
        for nbytes in (h * w * 4, fb):
            bufs.append(dev.DeviceBuffer(nbytes))
        dep, out = bufs
        for kind in cc.PLANES:
            z = cc.plane(kind, shape, n)
            dep.upload(z)
            for interp in cc.INTERPS:
                out.upload(fill)
                for first, count in cc.calls_of(run, n):
                    depth_render.composite_device(frames_dev[first:first + count], first, count, n, dep.ptr, out.ptr, h, w, dtype, interp)
                got = out.download(fill.shape, dtype)
                want = cc.expected(shape, n, dtype, kind, interp)
                name = (shape, n, cc.dtype_name(dtype), run, kind, interp)
                if kind == "integer":
                    assert got.tobytes() == want.tobytes(), name         # selected, never computed
                else:
                    assert cc.same_but_nan(got, want, cc.computed_nan(want, z, n, interp)), name
    finally:
        freed(bufs)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.dtype_name)
def test_composite_special_values_and_frame_ends(dev, dtype, shape):
    frames = cc.frames(shape, cc.N_SHORT, dtype)
    bufs = []
    try:
        for f in frames:
            bufs.append(dev.DeviceBuffer(f.nbytes))
            bufs[-1].upload(f)
        for run in ("whole", "chunks"):
            composite_run(dev, [b.ptr for b in bufs], shape, cc.N_SHORT, dtype, run)
        for b, f in zip(bufs, frames):
            assert b.download(f.shape, dtype).tobytes() == f.tobytes()
    finally:
        freed(bufs)


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.dtype_name)
def test_composite_128_frames_in_three_launches(dev, dtype):
    shape, n = cc.LONG_SHAPE, cc.N_LONG
    frames = cc.frames(shape, n, dtype)
    offs = cc.frame_offsets(shape, n, dtype, "slots")
    buf = dev.DeviceBuffer(offs[-1] + frames[0].nbytes)
    try:
        assert buf.ptr % 4 == 0
        for f, o in zip(frames, offs):
            buf.upload(f, o)
        composite_run(dev, [buf.ptr + o for o in offs], shape, n, dtype, "whole")
    finally:
        buf.free()


@pytest.mark.parametrize("every", [1, 2])
def test_composite_uint16_frames_off_a_word_boundary(dev, every):
    """every frame, then every second frame, 2 bytes past a 4-byte boundary: the gather path at uint16"""
    shape, n = cc.LONG_SHAPE, cc.N_SHORT
    frames = cc.frames(shape, n, np.uint16)
    offs = cc.frame_offsets(shape, n, np.uint16, "off %d" % every)
    buf = dev.DeviceBuffer(offs[-1] + frames[0].nbytes)
    try:
        for f, o in zip(frames, offs):
            buf.upload(f, o)
        ptrs = [buf.ptr + o for o in offs]
        assert buf.ptr % 4 == 0 and sum(p % 4 == 2 for p in ptrs) == (n if every == 1 else 3)
        for run in ("whole", "chunks"):
            composite_run(dev, ptrs, shape, n, np.uint16, run)
    finally:
        buf.free()


# ---------------------------------------------------------------- brush
def stroke_equals(rt, shape, dtype, points, brush):
    master, source = bc.frames(shape, dtype)
    out, area, layer = rt.stroke(master, source, list(points), *brush, return_mask=True)
    w_out, w_layer, w_area = bc.expected(shape, dtype, points, brush)
    assert layer.dtype == np.float64 and np.array_equal(layer, w_layer), (len(points), int((layer != w_layer).sum()))
    assert out.dtype == master.dtype and np.array_equal(out, w_out), (len(points), int((out != w_out).sum()))
    assert tuple(area) == w_area
    return layer


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_stroke_hit_counts_on_the_chunk_limits(dev, dtype):
    from shinestacker_amd import retouch
    for n in bc.HIT_COUNTS:
        layer = stroke_equals(retouch, bc.ONE_TILE_SHAPE, dtype, bc.one_tile_points(n), bc.ONE_TILE_BRUSH)
        assert 0 < layer.min() and layer.max() < 1, n


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_stroke_over_tiles_with_ragged_shares_of_the_blocks(dev, dtype):
    from shinestacker_amd import retouch
    layer = stroke_equals(retouch, bc.RAGGED_SHAPE, dtype, bc.ragged_points(), bc.RAGGED_BRUSH)
    assert layer.max() < 1
