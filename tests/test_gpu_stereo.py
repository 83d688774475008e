"""GPU: the stereo view kernel (csrc/kernels_stereo.hpp) against its NumPy restatement (tests/stereo_restatement.py), bit for
bit: the primitive on crafted depth planes, pair and rocking against compositions of restated views, and the stackers, the
pipeline and the actions feeding it their own depth map."""
import os

import numpy as np
import pytest

import stereo_restatement as sr
from conftest import GOLDEN, load_golden, stack_kwargs

pytestmark = pytest.mark.gpu

SEG = 512       # MI_SV_SEG: the targets a workgroup owns


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


def image(shape, dtype, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, tuple(shape) + (3,)).astype(dtype)


def depth_plane(kind, shape, n, seed=5):
    h, w = shape
    rng = np.random.default_rng(seed)
    if kind == "ramp":          # smooth, tilted, a little past both ends of the stack
        y, x = np.mgrid[0:h, 0:w]
        return (-0.01 + (n - 1 + 0.02) * ((x + 0.37 * y) / (w + 0.37 * h))).astype(np.float32)
    if kind == "steps":         # vertical steps between 0 and N - 1, at and next to the segment boundaries and elsewhere; a row
        z = np.zeros(shape, np.float32)     # shifts its steps by -2 .. 2 columns: the widest holes, the longest occlusions
        for y in range(h):
            edges = sorted({e + (y % 5) - 2 for e in list(range(SEG, w, SEG)) + [w // 3, (2 * w) // 3, 70, w - 70, SEG + 64, SEG - 64]}
                           & set(range(1, w)))
            val, prev = (y & 1) * (n - 1), 0
            for e in edges + [w]:
                z[y, prev:e] = val
                val, prev = (n - 1) - val, e
        return z
    if kind == "random":        # integer + fraction
        return (rng.integers(0, n, shape) + rng.random(shape) * 0.999).clip(0, n - 1).astype(np.float32)
    assert kind == "flat"
    return np.full(shape, 0.625 * (n - 1), np.float32)


# (5, 7): smaller than any segment; (37, 53), -7.5: ragged, and half-way products for rint (pivot 0.5, t in eighths and
# sixteenths on the random plane's integers and the flat plane); (3, 70), 64: a shift close to the width; (40, 600) +-64: two
# segments, sources and hole searches crossing the boundary; (8, 1100): three segments, a ragged last one; (131, 197): odd row
# lengths, so that rows start on every byte alignment of the 4-byte output words
CASES = [((5, 7), 2.0, 0.5, "last"), ((37, 53), -7.5, 0.5, "last"), ((3, 70), 64.0, 0.0, "last"), ((3, 70), -64.0, 0.5, "first"),
         ((40, 600), 64.0, 0.5, "last"), ((40, 600), -64.0, 0.3, "first"), ((8, 1100), 64.0, 1.0, "last"), ((131, 197), 24.0, 0.5, "last")]


@pytest.mark.parametrize("kind", ["ramp", "steps", "random", "flat"])
@pytest.mark.parametrize("shape,shift,pivot,near", CASES)
def test_view_equals_the_restatement(L, shape, shift, pivot, near, kind):
    from shinestacker_amd import stereo
    n = 9
    z = depth_plane(kind, shape, n, seed=shape[1])
    for dtype in (np.uint8, np.uint16):
        img = image(shape, dtype)
        got = stereo.view(img, z, n, shift, pivot, near)
        assert got.dtype == img.dtype and got.shape == img.shape
        assert np.array_equal(got, sr.view(img, z, n, shift, pivot, near)), dtype


@pytest.mark.parametrize("n", [1, 2, 4, 7])
def test_view_frame_counts(L, n):
    """N == 1: t = 0 whatever the depth says; N - 1 = 3, 6: the divide rounds"""
    from shinestacker_amd import stereo
    shape = (9, 140)
    z = depth_plane("random", shape, max(n, 2), seed=n)
    img = image(shape, np.uint16)
    for shift, pivot, near in ((33.0, 0.5, "last"), (-12.25, 0.0, "first"), (64.0, 1.0, "last")):
        assert np.array_equal(stereo.view(img, z, n, shift, pivot, near), sr.view(img, z, n, shift, pivot, near)), (shift, pivot, near)


def test_view_basics(L):
    from shinestacker_amd import stereo
    shape = (12, 700)
    img, z = image(shape, np.uint8), depth_plane("ramp", shape, 5)
    assert np.array_equal(stereo.view(img, z, 5, 0.0), img)
    got = stereo.view(img, np.full(shape, 4.0, np.float32), 5, 10.0, 0.5)         # a translation by +5
    assert np.array_equal(got[:, 5:], img[:, :-5]) and np.array_equal(got[:, :5], np.repeat(img[:, :1], 5, axis=1))
    # device form: a frame that does not start on a 4-byte boundary (a row of a contiguous stack), and its own output buffer
    fb = img.nbytes
    src, dep, out = L.DeviceBuffer(fb + 3), L.DeviceBuffer(z.nbytes), L.DeviceBuffer(fb + 3)
    try:
        src.upload(img, 3)
        dep.upload(z)
        stereo.view_device(src.ptr + 3, dep.ptr, out.ptr + 1, shape[0], shape[1], np.uint8, 5, -40.0, 0.25, "first")
        assert np.array_equal(out.download(img.shape, np.uint8, 1), sr.view(img, z, 5, -40.0, 0.25, "first"))
        with pytest.raises(ValueError):
            stereo.view_device(src.ptr, dep.ptr, src.ptr, shape[0], shape[1], np.uint8, 5, 4.0)
    finally:
        for b in (src, dep, out):
            b.free()


@pytest.mark.parametrize("dtype,shape", [(np.uint8, (37, 53)), (np.uint16, (37, 53)), (np.uint8, (5, 7)), (np.uint16, (6, 530))])
def test_pair_and_rocking(L, dtype, shape):
    from shinestacker_amd import stereo
    n = 6
    sep = 5.0 if shape[1] < 10 else 21.0
    img, z = image(shape, dtype, 3), depth_plane("random", shape, n)
    left, right = sr.view(img, z, n, np.float32(sep / 2), 0.4, "first"), sr.view(img, z, n, np.float32(-sep / 2), 0.4, "first")
    ana = right.copy()
    ana[:, :, 2] = left[:, :, 2]
    for layout, want in (("parallel", np.concatenate([left, right], axis=1)), ("cross", np.concatenate([right, left], axis=1)),
                         ("anaglyph", ana)):
        got = stereo.pair(img, z, n, sep, 0.4, "first", layout)
        assert got.dtype == img.dtype and np.array_equal(got, want), layout
        assert np.array_equal(want, sr.pair(img, z, n, sep, 0.4, "first", layout))
    frames = stereo.rocking(img, z, n, sep, views=5)
    want = sr.rocking(img, z, n, sep, views=5)
    assert len(frames) == 5 and all(np.array_equal(a, b) for a, b in zip(frames, want))
    assert np.array_equal(frames[0], sr.view(img, z, n, -sep / 2)) and np.array_equal(frames[-1], sr.view(img, z, n, sep / 2))
    assert np.array_equal(stereo.pair(img, z, n, sep)[:, :shape[1]], frames[-1])         # the defaults: parallel, left first


# ------------------------------------------------------------------ the stackers' own depth maps
@pytest.mark.parametrize("case", ["g1_u8", "g2_u16"])
def test_pyramid_stack_depth_map_into_a_pair(L, case):
    from shinestacker_amd import PyramidStack, stereo
    g = load_golden(case)
    algo = PyramidStack(**stack_kwargs(g["params"]))
    try:
        fused = algo.focus_stack_arrays(list(g["frames"]))
        depth = algo.depth_map()
        n = len(g["frames"])
        assert depth.max() > depth.min()
        for layout in ("anaglyph", "parallel"):
            assert np.array_equal(stereo.pair(fused, depth, n, 12.0, layout=layout), sr.pair(fused, depth, n, 12.0, layout=layout))
        assert not np.array_equal(stereo.view(fused, depth, n, 6.0), fused)
    finally:
        algo.close()


def test_depth_map_stack_depth_map_into_a_view(L):
    from shinestacker_amd import DepthMapStack, stereo
    g = load_golden("g1_u8")
    algo = DepthMapStack()
    try:
        fused = algo.focus_stack_arrays(list(g["frames"]))
        depth = algo.depth_map()
        n = len(g["frames"])
        assert np.array_equal(stereo.view(fused, depth, n, -9.0, near="first"), sr.view(fused, depth, n, -9.0, near="first"))
    finally:
        algo.close()


# ------------------------------------------------------------------ pipeline and actions
def _synth(L, n, h, w):
    dev = L.DeviceBuffer(n * h * w * 3)
    try:
        L.synth_frames_device(dev.ptr, np.uint8, h, w, 0, n, n)
        return list(dev.download((n, h, w, 3), np.uint8))
    finally:
        dev.free()


def _identity(a, b, *_cfg):
    return 100, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


@pytest.mark.parametrize("extra", [{}, {"unsharp": (1.0, 1.0, 0.0)}])
def test_align_and_stack_returns_the_pair(L, extra):
    from shinestacker_amd import pipeline, stereo
    n, h, w = 4, 96, 160
    frames = _synth(L, n, h, w)
    info = {}
    img, _ = pipeline.align_and_stack(frames, estimator=_identity, depth_map=True, stereo=dict(separation=12.0), info=info, **extra)
    img0, _ = pipeline.align_and_stack(frames, estimator=_identity, **extra)
    assert np.array_equal(img, img0)                    # the returned image is the same with and without stereo=
    got = info["stereo"]
    assert got.shape == (h, w, 3) and got.dtype == np.uint8
    assert np.array_equal(got, stereo.pair(img, info["depth_map"], n, 12.0, layout="anaglyph"))
    assert np.array_equal(got, sr.pair(img, info["depth_map"], n, 12.0, layout="anaglyph"))
    assert not np.array_equal(got, img)
    # its own sigma and a side-by-side layout, without depth_map=
    info2 = {}
    pipeline.align_and_stack(frames, estimator=_identity, stereo=dict(layout="cross", separation=8, pivot=0.25, near="first", sigma=0.0),
                             info=info2, **extra)
    info3 = {}
    pipeline.align_and_stack(frames, estimator=_identity, depth_map=0.0, info=info3, **extra)
    assert "depth_map" not in info2 and "stereo" not in info3
    assert np.array_equal(info2["stereo"], sr.pair(img, info3["depth_map"], n, 8, 0.25, "first", "cross"))


def test_align_and_stack_device_returns_the_pair(L):
    from shinestacker_amd import pipeline
    n, h, w = 8, 96, 160
    fb = h * w * 3
    frames, out_dev = L.DeviceBuffer(n * fb), L.DeviceBuffer(fb)
    try:
        L.synth_frames_device(frames.ptr, np.uint8, h, w, 0, n, n)
        info = {}
        img, tr, cc = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, depth_map=2.0, stereo=dict(separation=20.0), info=info)
        img0, tr0, cc0 = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8)
        assert np.array_equal(img, img0) and cc == cc0
        assert np.array_equal(info["stereo"], sr.pair(img, info["depth_map"], n, 20.0, layout="anaglyph"))
        # with out_dev the frame stays on the device; the pair is still an array
        info_d = {}
        res = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, stereo=dict(separation=20.0, layout="parallel"), info=info_d,
                                              out_dev=out_dev.ptr)
        assert res[0] is None and np.array_equal(out_dev.download((h, w, 3), np.uint8), img)
        assert np.array_equal(info_d["stereo"], sr.pair(img, info["depth_map"], n, 20.0, layout="parallel"))
        info_n = {}
        pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, info=info_n)
        assert "stereo" not in info_n
    finally:
        frames.free()
        out_dev.free()


def _run_focus_stack(tmp_path, name, **kw):
    import shutil
    from shinestacker_amd import FocusStack, PyramidStack, StackJob
    work = tmp_path / name
    (work / "src").mkdir(parents=True)
    for fn in sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop"))):
        shutil.copy(os.path.join(GOLDEN, "img_jpg_crop", fn), work / "src" / fn)
    algo = PyramidStack()
    job = StackJob("job", str(work), input_path="src")
    job.add_action(FocusStack("stack", algo, **kw))
    job.run()
    return work, algo


def test_focus_stack_writes_the_stereo_pair(L, tmp_path):
    from shinestacker_amd import stereo
    from shinestacker_amd.imageio import read_img
    work, algo = _run_focus_stack(tmp_path, "with", stereo_path="stereo")
    try:
        stacked = read_img(str(work / "stack" / "stack_0000.png"))
        written = work / "stereo" / "stack_0000.png"
        assert written.is_file()
        want = sr.pair(stacked, algo.depth_map(), 6, stereo.DEFAULT_SEPARATION, layout="anaglyph")
        assert np.array_equal(read_img(str(written)), want) and not np.array_equal(want, stacked)
    finally:
        algo.close()
    plain, algo2 = _run_focus_stack(tmp_path, "without")
    algo2.close()
    assert not (plain / "stereo").exists()
    assert np.array_equal(stacked, read_img(str(plain / "stack" / "stack_0000.png")))
    # the other options, and depth_map_sigma without depth_map_path
    work2, algo3 = _run_focus_stack(tmp_path, "options", stereo_path="3d", stereo_layout="parallel", stereo_separation=40,
                                    stereo_pivot=0.0, stereo_near="first", depth_map_sigma=0.0)
    try:
        want = sr.pair(stacked, algo3.depth_map(0.0), 6, 40, 0.0, "first", "parallel")
        assert np.array_equal(read_img(str(work2 / "3d" / "stack_0000.png")), want)
        assert not (work2 / "depth").exists()
    finally:
        algo3.close()
