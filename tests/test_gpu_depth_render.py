"""GPU: the depth-selected composite -- depth_composite_kernel (csrc/kernels_composite.hpp) behind depth_render.composite /
composite_device, the pipeline's depth_composite= and the action's depth_composite_path= -- every comparison is array_equal
against the NumPy restatement (tests/depth_render_restatement.py), no tolerances."""
import os
import shutil

import numpy as np
import pytest

import brush_restatement as br
import depth_render_restatement as dr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (33, 130), (64, 257), (130, 1030)]
COUNTS = [1, 2, 5, 40]
DTYPES = [np.uint8, np.uint16, np.float32]
SENTINEL = {np.uint8: 0xA5, np.uint16: 0xA5C3, np.float32: -12345.678}


@pytest.fixture(scope="module")
def render(hiplib):
    hiplib.require_device()
    from shinestacker_amd import depth_render
    return depth_render


def make_frames(shape, n, dtype, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if dtype == np.float32:     # not small integers: negative, fractional, 1e6 scale
        return [((rng.random(shape + (3,)) - 0.5) * 2.0e6).astype(np.float32) for _ in range(n)]
    return [rng.integers(0, np.iinfo(dtype).max + 1, shape + (3,)).astype(dtype) for _ in range(n)]


def planes(shape, n, seed=0):
    """the depth planes of one shape and stack length, by name"""
    h, w = shape
    rng = np.random.default_rng(2000 + seed)
    rand = np.array(rng.random(shape) * (n + 1) - 1, np.float32)            # fractional over [-1, N]
    rand[rng.random(shape) < 0.03] = np.nan
    ties = np.array([0.5, 1.5, 2.5, 0.0, n - 1, n - 0.5, -0.5, n + 3.0, np.nan, np.inf, -np.inf, 1.0, 2.0, 0.25], np.float32)
    tie = np.resize(ties, shape).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.where((yy + xx) % 2 == 0, 0.0, float(n - 1)).astype(np.float32)
    half = np.full(shape, float(min(1, n - 1)), np.float32)                 # uniform on the left half of every row, mixed on the right
    half[:, w // 2:] = rand[:, w // 2:]
    flat = rand.copy()                                                      # uniform over whole runs of 256 flat pixels, mixed between
    flat.reshape(-1)[: (h * w) // 2] = np.float32(min(n - 1, 1) * 0.75 + (n > 2))
    return {"random": rand, "ties": tie, "const_int": np.full(shape, float(n // 2), np.float32),
            "const_frac": np.full(shape, np.float32(max(n - 1, 0) * 0.37), np.float32), "checker": checker, "half": half, "flat": flat}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_plane_equals_the_restatement(render, shape, dtype):
    """one upload of the frames per stack length; both interp over every plane; the inputs are only read"""
    from shinestacker_amd import _lib
    h, w = shape
    for n in COUNTS:
        frames = make_frames(shape, n, dtype, n)
        bufs = [_lib.DeviceBuffer(f.nbytes) for f in frames]
        dep, out = _lib.DeviceBuffer(h * w * 4), _lib.DeviceBuffer(frames[0].nbytes)
        try:
            for b, f in zip(bufs, frames):
                b.upload(f)
            for name, plane in planes(shape, n, n).items():
                dep.upload(plane)
                for interp in ("linear", "nearest"):
                    out.upload(np.full_like(frames[0], SENTINEL[dtype]))
                    render.composite_device([b.ptr for b in bufs], 0, n, n, dep.ptr, out.ptr, h, w, dtype, interp)
                    got = out.download(frames[0].shape, dtype)
                    want = dr.composite(frames, plane, interp)
                    assert got.tobytes() == want.tobytes(), (n, name, interp, int((got != want).sum()))
                assert dep.download(shape, np.float32).tobytes() == plane.tobytes(), (n, name)
            for b, f in zip(bufs, frames):
                assert np.array_equal(b.download(f.shape, dtype), f)
        finally:
            for b in bufs + [dep, out]:
                b.free()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_chunks_over_one_output(render, dtype, interp):
    """calls over chunks of 2 and of 3 frames into one output prefilled with a sentinel equal the one-call result, which has no
    sentinel left; a single middle chunk leaves every pixel it does not own at the sentinel"""
    from shinestacker_amd import _lib
    shape, n = (33, 130), 5
    h, w = shape
    frames = make_frames(shape, n, dtype, 7)
    bufs = [_lib.DeviceBuffer(f.nbytes) for f in frames]
    dep, out = _lib.DeviceBuffer(h * w * 4), _lib.DeviceBuffer(frames[0].nbytes)
    fill = np.full_like(frames[0], SENTINEL[dtype])
    try:
        for b, f in zip(bufs, frames):
            b.upload(f)
        for name in ("random", "ties", "half"):
            plane = planes(shape, n, 7)[name]
            dep.upload(plane)
            whole = dr.composite(frames, plane, interp)
            for other in (fill, np.full_like(fill, 1)):     # the same frame over two different fills: no sample of a fill is left
                out.upload(other)
                render.composite_device([b.ptr for b in bufs], 0, n, n, dep.ptr, out.ptr, h, w, dtype, interp)
                assert out.download(fill.shape, dtype).tobytes() == whole.tobytes()
            for size in (2, 3):
                out.upload(fill)
                for first, count in dr.chunks(n, size):
                    render.composite_device([b.ptr for b in bufs[first:first + count]], first, count, n, dep.ptr, out.ptr, h, w, dtype, interp)
                assert out.download(fill.shape, dtype).tobytes() == whole.tobytes(), (name, size)
            out.upload(fill)
            render.composite_device([b.ptr for b in bufs[2:4]], 2, 2, n, dep.ptr, out.ptr, h, w, dtype, interp)
            got = out.download(fill.shape, dtype)
            mine = dr.indices(plane, n)[1] == 2
            assert mine.any() and (got[~mine] == fill[~mine]).all() and got[mine].tobytes() == whole[mine].tobytes()
    finally:
        for b in bufs + [dep, out]:
            b.free()


def test_frames_off_a_word_boundary_take_the_gather_path(render):
    """uint8 frames packed back to back with an odd byte size, as a resident stack holds them: every second frame starts off a
    4-byte boundary, and a constant plane still gives the restatement"""
    from shinestacker_amd import _lib
    shape, n = (5, 7), 4
    frames = make_frames(shape, n, np.uint8, 9)
    fb = frames[0].nbytes
    assert fb % 4
    buf, dep, out = _lib.DeviceBuffer(fb * n), _lib.DeviceBuffer(5 * 7 * 4), _lib.DeviceBuffer(fb)
    try:
        buf.upload(np.stack(frames))
        for d in (1.0, 1.5, 2.25):
            plane = np.full(shape, d, np.float32)
            dep.upload(plane)
            for interp in ("linear", "nearest"):
                render.composite_device([buf.ptr + i * fb for i in range(n)], 0, n, n, dep.ptr, out.ptr, 5, 7, np.uint8, interp)
                assert np.array_equal(out.download(frames[0].shape, np.uint8), dr.composite(frames, plane, interp))
    finally:
        for b in (buf, dep, out):
            b.free()


def test_more_frames_than_one_launch_holds(render):
    """a launch carries 64 frame addresses: 65 (a last sub-chunk of exactly 2), 70 and 127 frames in one call"""
    from shinestacker_amd import _lib
    shape = (9, 31)
    for n in (64, 65, 70, 127):
        frames = make_frames(shape, n, np.uint16, n)
        fb = frames[0].nbytes
        buf, dep, out = _lib.DeviceBuffer(fb * n), _lib.DeviceBuffer(9 * 31 * 4), _lib.DeviceBuffer(fb)
        try:
            buf.upload(np.stack(frames))
            for name in ("random", "ties", "checker"):
                plane = planes(shape, n, n)[name]
                dep.upload(plane)
                for interp in ("linear", "nearest"):
                    out.upload(np.full_like(frames[0], 0xA5C3))
                    render.composite_device([buf.ptr + i * fb for i in range(n)], 0, n, n, dep.ptr, out.ptr, 9, 31, np.uint16, interp)
                    assert np.array_equal(out.download(frames[0].shape, np.uint16), dr.composite(frames, plane, interp)), (n, name, interp)
        finally:
            for b in (buf, dep, out):
                b.free()


def test_an_output_that_aliases_a_frame_is_refused(render, hiplib):
    from shinestacker_amd import _lib
    bufs = [_lib.DeviceBuffer(4 * 8 * 3) for _ in range(2)]
    dep = _lib.DeviceBuffer(4 * 8 * 4)
    try:
        with pytest.raises(ValueError, match="alias"):
            render.composite_device([b.ptr for b in bufs], 0, 2, 2, dep.ptr, bufs[1].ptr, 4, 8, np.uint8)
        with pytest.raises(ValueError):
            render.composite_device([b.ptr for b in bufs], 0, 2, 2, dep.ptr, dep.ptr, 4, 8, np.uint8)
    finally:
        for b in bufs + [dep]:
            b.free()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_composite_from_a_generator_in_chunks_of_two(render, dtype):
    shape, n = (33, 130), 5
    frames = make_frames(shape, n, dtype, 11)
    keep = [f.copy() for f in frames]
    for name in ("random", "ties"):
        plane = planes(shape, n, 11)[name]
        for interp in ("linear", "nearest"):
            whole = render.composite(frames, plane, interp)
            assert whole.tobytes() == dr.composite(frames, plane, interp).tobytes()
            assert render.composite((f for f in frames), plane, interp, resident=2).tobytes() == whole.tobytes()
            assert render.composite(iter(frames), plane, interp, resident=3).tobytes() == whole.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(frames, keep))
    assert np.array_equal(render.composite([frames[0]], planes(shape, 1, 11)["random"]), frames[0])
    from shinestacker_amd import BitDepthError, ShapeError
    with pytest.raises(ShapeError):
        render.composite([frames[0], frames[1][:-1]], planes(shape, 2, 11)["random"])
    with pytest.raises(BitDepthError):
        render.composite([frames[0], frames[1].astype(np.float64)], planes(shape, 2, 11)["random"])


def test_host_form_of_the_abi(render, hiplib):
    import ctypes as C
    shape, n = (33, 130), 5
    frames = make_frames(shape, n, np.uint16, 13)
    plane = planes(shape, n, 13)["random"]
    out = np.full_like(frames[0], 7)
    tab = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    hiplib.check(hiplib.load().mi_depth_composite(0, tab, 0, n, n, plane.ctypes.data, out.ctypes.data, shape[0], shape[1], hiplib.MI_U16, 0))
    assert np.array_equal(out, dr.composite(frames, plane, "linear"))


# ------------------------------------------------------------------------------------------------ pipeline and action
def test_pipeline_renders_the_frames_as_they_were_pushed(hiplib, render):
    """the frames and the estimator of test_gpu_brush.py::test_pipeline_paints_from_the_frames_as_they_were_pushed"""
    from shinestacker_amd import Stroke, retouch as rt
    from shinestacker_amd.align import _BORDER_CODE, _DEFAULT_ALIGNMENT_CONFIG
    from shinestacker_amd.imageio import read_img
    from shinestacker_amd.pipeline import align_and_stack
    names = sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop")))
    fr = [read_img(os.path.join(GOLDEN, "img_jpg_crop", n)) for n in names]
    h, w = fr[0].shape[:2]
    ref_idx = len(fr) // 2
    mats = [np.array([[1.0, 0.0, 0.75 * (i + 1)], [0.0, 1.0, -0.5 * i - 0.25]]) for i in range(len(fr))]

    def est(i0, i1, fc, mc, ac):
        i = next(k for k, f in enumerate(fr) if np.array_equal(f, i0))
        assert np.array_equal(i1, fr[ref_idx])
        return 500, mats[i]
    kw = dict(estimator=est, alignment_config={'subsample': 1})
    cfg = _DEFAULT_ALIGNMENT_CONFIG
    pushed = [f if i == ref_idx else hiplib.warp_affine(f, mats[i], _BORDER_CODE[cfg['border_mode']], cfg['border_value'], 21, cfg['border_blur'])
              for i, f in enumerate(fr)]
    s = 1.5
    plain, m_plain = align_and_stack(fr, **kw)
    for interp in ("linear", "nearest"):
        d = {}
        got, m = align_and_stack(fr, depth_composite={"interp": interp}, depth_map=s, info=d, **kw)
        assert np.array_equal(got, plain) and m == m_plain
        assert d["depth_map"].shape == (h, w) and np.array_equal(d["depth_composite"], dr.composite(pushed, d["depth_map"], interp))
    assert not np.array_equal(d["depth_composite"], plain)
    d0 = {}
    got, m = align_and_stack(fr, depth_composite=None, depth_map=s, info=d0, **kw)
    assert np.array_equal(got, plain) and m == m_plain and "depth_composite" not in d0
    strokes = [Stroke("depth_composite", rt.stamps_along([(10, 10), (w - 10, h // 2)], 41), 41, 50, 100, 80),
               Stroke(ref_idx, rt.stamps_along([(w // 2, -5), (w // 3, h + 5)], 25), 25, 0, 100, 100)]
    d2 = {}
    painted, _ = align_and_stack(fr, depth_composite={"interp": "linear"}, depth_map=s, retouch=strokes, info=d2, **kw)
    comp = dr.composite(pushed, d2["depth_map"], "linear")
    assert np.array_equal(d2["depth_composite"], comp)
    wanted = plain
    for st, src in zip(strokes, (comp, fr[ref_idx])):
        r = br.radius_of(st.size)
        wanted = br.stroke_fold(wanted, src, rt.brush_mask(2 * r + 1, st.hardness, st.opacity), br.centres(st.points), r, st.opacity, st.flow)[0]
    assert np.array_equal(painted, wanted) and not np.array_equal(painted, plain)


def test_device_pipeline_gathers_the_resident_frames(hiplib, render):
    """align_and_stack_device(depth_composite=...): the result, the transforms and the coefficients of the plain call, and a
    DeviceBuffer that holds the restatement's composite of the aligned frames -- read back from the kept handles' buffer, where
    the kernel gathered them without a copy -- by the depth map the same call returns; refused when the frames pass in more
    than one push"""
    from shinestacker_amd import InvalidOptionError, _lib
    from shinestacker_amd.pipeline import align_and_stack_device
    n, h, w = 8, 96, 160
    fb = h * w * 3
    buf = _lib.DeviceBuffer(fb * n)
    try:
        hiplib.synth_frames_device(buf.ptr, np.uint8, h, w, 0, n, n)
        for kw in ({}, {"step_process": True}):
            plain, t0, c0 = align_and_stack_device(buf.ptr, n, h, w, np.uint8, **kw)
            for interp in ("linear", "nearest"):
                d = {}
                got, t1, c1, hd = align_and_stack_device(buf.ptr, n, h, w, np.uint8, depth_composite={"interp": interp}, depth_map=True,
                                                         info=d, keep_handles=True, **kw)
                comp = d["depth_composite"]
                try:
                    assert isinstance(comp, _lib.DeviceBuffer) and comp.nbytes == fb
                    img = comp.download((h, w, 3), np.uint8)
                    pushed = hd.batches.download((n, h, w, 3), np.uint8)
                finally:
                    comp.free()
                    hd.close()
                assert np.array_equal(got, plain) and c1 == c0
                assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(t1, t0))
                assert np.array_equal(img, dr.composite(list(pushed), d["depth_map"], interp))
        d = {}
        align_and_stack_device(buf.ptr, n, h, w, np.uint8, depth_composite=None, info=d)
        assert "depth_composite" not in d
        with pytest.raises(InvalidOptionError):
            align_and_stack_device(buf.ptr, n, h, w, np.uint8, depth_composite={}, info={}, batch_frames=4)
    finally:
        buf.free()


def test_focus_stack_action_writes_the_composite(hiplib, render, tmp_path):
    from shinestacker_amd import FocusStack, PyramidStack, StackJob
    from shinestacker_amd.imageio import read_img
    src = os.path.join(GOLDEN, "img_jpg_crop")
    names = sorted(os.listdir(src))
    os.makedirs(tmp_path / "input")
    for n in names:
        shutil.copy(os.path.join(src, n), tmp_path / "input" / n)
    fr = [read_img(os.path.join(src, n)) for n in names]
    outs = {}
    for key, extra in (("plain", {}), ("with", dict(depth_composite_path="composite", depth_composite_interp="linear"))):
        job = StackJob("job", str(tmp_path), input_path="input")
        algo = PyramidStack()
        job.add_action(FocusStack("stack", algo, output_path="out-" + key, prefix="p_", **extra))
        job.run()
        if key == "plain":
            assert not os.path.exists(tmp_path / "composite")
        outs[key] = (read_img(os.path.join(str(tmp_path), "out-" + key, "p_" + names[0])), algo)
    assert np.array_equal(outs["plain"][0], outs["with"][0])
    name, algo = "p_" + names[0], outs["with"][1]
    want = render.composite(fr, algo.depth_map(), "linear")
    assert np.array_equal(want, dr.composite(fr, algo.depth_map(), "linear"))
    got = read_img(str(tmp_path / "composite" / name))
    # the file is a JPEG like its inputs: it is compared with the wanted frame through the same writer
    from shinestacker_amd.imageio import write_img
    write_img(str(tmp_path / ("want_" + name)), want)
    assert np.array_equal(got, read_img(str(tmp_path / ("want_" + name))))
