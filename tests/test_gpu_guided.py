"""GPU: the depth refinement (csrc/kernels_guided.hpp) against its NumPy restatement (tests/guided_restatement.py), bit for bit:
mi_depth_guided and its device form on the whole case table of tests/guided_cases.py, the refined depth maps of PyramidStack
and DepthMapStack against the restatement fed with the unrefined map, the handle's own weight plane and the fused frame, and
the depth_refine= option of the pipeline and of FocusStack."""
import os

import numpy as np
import pytest

import guided_cases as gc
import guided_restatement as gr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

REFINE = {"radius": 6, "eps": 1e-4}
WIDE = {"radius": 32, "eps": 1e-2}


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


def differing(got, want):
    return int((got != want).sum()), np.argwhere(got != want)[:5].tolist()


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case", gc.TABLE, ids=gc.case_name)
def test_guided_refine_equals_the_restatement(L, case):
    from shinestacker_amd import depth_out
    p, w, g = gc.planes(case)
    lo, hi = gc.limits(case)
    want = gc.expected(case)
    got = depth_out.guided_refine(p, w, g, case.radius, gc.EPS, lo, hi)
    assert got.dtype == np.float32 and got.shape == case.shape
    assert got.tobytes() == want.tobytes(), differing(got, want)
    # the device form, with guard values around the output plane and a scratch buffer of exactly the stated size
    h, wd = case.shape
    guard = np.full(h * wd + 8, -77.0, np.float32)
    bufs = [L.DeviceBuffer(n) for n in (p.nbytes, w.nbytes, g.nbytes, guard.nbytes, depth_out.SCRATCH_PLANES * h * wd * 8)]
    try:
        dp, dw, dg, dout, scratch = bufs
        dp.upload(p)
        dw.upload(w)
        dg.upload(g)
        dout.upload(guard)
        depth_out.guided_refine_device(dp.ptr, dw.ptr, w.dtype, dg.ptr, g.dtype, h, wd, dout.ptr + 16, lo, hi, case.radius, gc.EPS,
                                       scratch_ptr=scratch.ptr)
        L.check(L.load().mi_device_synchronize(0))
        back = dout.download(guard.shape, np.float32)
        assert back[4:-4].tobytes() == want.tobytes(), differing(back[4:-4].reshape(case.shape), want)
        assert (back[:4] == -77.0).all() and (back[-4:] == -77.0).all()
        assert dp.download(p.shape, np.float32).tobytes() == p.tobytes() and dg.download(g.shape, g.dtype).tobytes() == g.tobytes()
    finally:
        for b in bufs:
            b.free()


def test_defaults_and_the_scratch_the_binding_makes(L):
    from shinestacker_amd import depth_out
    case = gc.TABLE[-4]
    p, w, g = gc.planes(case)
    got = depth_out.guided_refine(p, w, g)          # radius 6, eps 1e-4, lo / hi the map's own range
    assert np.array_equal(got, gr.guided_refine(p, w, g, 6, 1e-4, float(p.min()), float(p.max())))
    h, wd = case.shape
    bufs = [L.DeviceBuffer(n) for n in (p.nbytes, w.nbytes, g.nbytes, p.nbytes)]
    try:
        for b, a in zip(bufs, (p, w, g)):
            b.upload(a)
        depth_out.guided_refine_device(bufs[0].ptr, bufs[1].ptr, w.dtype, bufs[2].ptr, g.dtype, h, wd, bufs[3].ptr, float(p.min()),
                                       float(p.max()))
        assert np.array_equal(bufs[3].download(p.shape, np.float32), got)
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------------------------------ the stackers
def stack_frames(n=8, shape=(70, 90), dtype=np.uint8, seed=3):
    """`n` frames, each sharp (noise) in its own band of columns and smooth elsewhere, on a dark / bright step"""
    h, w = shape
    rng = np.random.default_rng(seed)
    top = 255 if dtype == np.uint8 else 65535
    y, x = np.mgrid[:h, :w]
    base = np.where(x < w // 2, 0.3, 0.7) + 0.1 * np.sin(y / 9.0)
    out = []
    for i in range(n):
        noise = rng.normal(0.0, 0.12, (h, w, 3))
        sharp = ((x * n) // w == i)[:, :, None]
        out.append(np.rint(np.clip(base[:, :, None] + np.where(sharp, noise, noise / 30.0), 0, 1) * top).astype(dtype))
    return out


@pytest.mark.parametrize("float_type,first,stride", [("f32", 0, 1), ("f64", 0, 1), ("f32", 3, 2), ("f64", 5, 3)])
def test_pyramid_stack_refined_depth_map(L, float_type, first, stride):
    frames = stack_frames()
    n, (h, w) = len(frames), frames[0].shape[:2]
    st = L.Stack(h, w, in_dtype=np.uint8, float_type=L.MI_F64 if float_type == "f64" else L.MI_F32, arith="exact")
    try:
        if (first, stride) != (0, 1):
            st.set_first_index(first, stride=stride)
        for f in frames:
            st.push_frame(f)
        fused = st.finish()
        en = st.tap(L.TAP_ENERGY, 0)
        lo, hi = first, first + (n - 1) * stride
        for sigma, opts in ((0.0, REFINE), (2.0, REFINE), (0.0, WIDE)):
            plain = st.depth_map(sigma)
            want = gr.guided_refine(plain, en, fused, opts["radius"], opts["eps"], lo, hi)
            got = st.depth_map(sigma, refine=opts, guide=fused)
            assert got.dtype == np.float32 and np.array_equal(got, want), (sigma, differing(got, want))
            assert lo <= got.min() and got.max() <= hi and not np.array_equal(got, plain)
            assert np.array_equal(st.depth_map(sigma), plain)            # the state is read only
            gbuf, obuf = L.DeviceBuffer(fused.nbytes), L.DeviceBuffer(got.nbytes)
            try:
                gbuf.upload(fused)
                assert st.depth_map(sigma, obuf.ptr, refine=opts, guide=(gbuf.ptr, fused.dtype)) is None
                assert np.array_equal(obuf.download(got.shape, np.float32), want)
            finally:
                gbuf.free()
                obuf.free()
        assert np.array_equal(st.tap(L.TAP_ENERGY, 0), en)
    finally:
        st.close()


@pytest.mark.parametrize("float_type", ["float-32", "float-64"])
def test_pyramid_stacker_refines_against_its_own_fused_frame(L, float_type):
    from shinestacker_amd import InvalidOptionError, PyramidStack
    frames = stack_frames(dtype=np.uint16)
    algo = PyramidStack(float_type=float_type, min_size=16)
    try:
        with pytest.raises(RuntimeError):
            algo.depth_map(0.0, refine=REFINE)              # no stack yet: as the unrefined call
        fused = algo.focus_stack_arrays(frames)
        en = algo._stack.tap(L.TAP_ENERGY, 0)
        for sigma in (0.0, 2.0):
            got = algo.depth_map(sigma, refine=REFINE)
            want = gr.guided_refine(algo.depth_map(sigma), en, fused, 6, 1e-4, 0, len(frames) - 1)
            assert np.array_equal(got, want), (sigma, differing(got, want))
        assert np.array_equal(algo.depth_map(refine={}), algo.depth_map(2.0, refine=REFINE))      # the defaults of both
        buf = L.DeviceBuffer(got.nbytes)
        try:
            assert algo.depth_map(2.0, buf.ptr, refine=REFINE) is None
            assert np.array_equal(buf.download(got.shape, np.float32), got)
        finally:
            buf.free()
        with pytest.raises(InvalidOptionError):
            algo.depth_map(0.0, refine={"radius": 40})
        with pytest.raises(InvalidOptionError):
            algo.depth_map(0.0, refine={"window": 3})
    finally:
        algo.close()


@pytest.mark.parametrize("kw", [{}, {"map_type": "max"}, {"float_type": "float-64", "smooth_size": 0},
                                {"float_type": "float-64", "map_type": "max", "smooth_size": 0}],
                         ids=["average", "max", "average f64", "max f64"])
def test_depth_map_stack_refined_depth_map(L, kw):
    from shinestacker_amd import DepthMapStack
    frames = stack_frames()
    dms = DepthMapStack(**kw)
    try:
        with pytest.raises(RuntimeError):
            dms.depth_map(refine=REFINE)
        fused = dms.focus_stack_arrays(frames)
        tot = dms._dmap.tap(L.DM_TAP_TOTAL)
        assert tot.dtype == (np.float64 if "float_type" in kw else np.float32)
        weight = tot if kw.get("map_type", "average") == "average" else np.ones(tot.shape, tot.dtype)
        for sigma in (0.0, 2.0):
            plain = dms.depth_map(sigma)
            want = gr.guided_refine(plain, weight, fused, 6, 1e-4, 0, len(frames) - 1)
            got = dms.depth_map(sigma, refine=REFINE)
            assert got.dtype == np.float32 and np.array_equal(got, want), (sigma, differing(got, want))
            assert not np.array_equal(got, plain) and np.array_equal(dms.depth_map(sigma), plain)
        buf = L.DeviceBuffer(got.nbytes)
        try:
            assert dms.depth_map(2.0, buf.ptr, refine=REFINE) is None
            assert np.array_equal(buf.download(got.shape, np.float32), got)
        finally:
            buf.free()
        assert np.array_equal(dms._dmap.tap(L.DM_TAP_TOTAL), tot)
    finally:
        dms.close()


def test_handle_forms_report_state_and_arguments(L):
    g = np.zeros((64, 80, 3), np.uint8)
    out = np.empty((64, 80), np.float32)
    lib = L.load()
    st = L.Stack(64, 80)
    try:
        assert lib.mi_stack_depth_map_refined(st._h, 0.0, g.ctypes.data, L.MI_U8, 6, 1e-4, out.ctypes.data) == L.MI_ERR_STATE
        assert lib.mi_stack_depth_map(st._h, 0.0, out.ctypes.data) == L.MI_ERR_STATE
        st.push_frame(g)
        assert lib.mi_stack_depth_map_refined(st._h, 0.0, g.ctypes.data, L.MI_U8, 0, 1e-4, out.ctypes.data) == L.MI_ERR_INVALID
        assert b"radius" in lib.mi_last_error()
        assert lib.mi_stack_depth_map_refined(st._h, 17.0, g.ctypes.data, L.MI_U8, 6, 1e-4, out.ctypes.data) == L.MI_ERR_INVALID
        assert b"sigma" in lib.mi_last_error()
        got = st.depth_map(0.0, refine=REFINE, guide=g)         # one flat frame: index 0 everywhere, lo = hi = 0
        assert np.array_equal(got, np.zeros((64, 80), np.float32))
    finally:
        st.close()
    d = L.DepthMap(64, 80)
    try:
        d.push_frame(g)
        assert lib.mi_dmap_depth_map_refined(d._h, 0.0, g.ctypes.data, L.MI_U8, 6, 1e-4, out.ctypes.data) == L.MI_ERR_STATE
        assert lib.mi_dmap_depth_map_refined(d._h, 0.0, g.ctypes.data, L.MI_U8, 6, 0.0, out.ctypes.data) == L.MI_ERR_INVALID
    finally:
        d.close()


# ------------------------------------------------------------------ the pipeline
def identity(a, b, *_cfg):
    return 100, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def test_align_and_stack_refines_every_depth_map(L):
    from shinestacker_amd import InvalidOptionError, depth_render, pipeline, stereo
    from shinestacker_amd.align import _BORDER_CODE, _DEFAULT_ALIGNMENT_CONFIG as cfg
    frames = stack_frames(n=6, shape=(64, 96))
    n = len(frames)
    # what the pipeline pushes: every frame but the reference passes through the warp, here with the identity
    pushed = [f if i == n // 2 else L.warp_affine(f, identity(f, f)[1], _BORDER_CODE[cfg['border_mode']], cfg['border_value'], 21,
                                                  cfg['border_blur']) for i, f in enumerate(frames)]
    sv, dc = {"layout": "parallel", "separation": 3.0}, {"interp": "linear"}
    info, plain = {}, {}
    img, _ = pipeline.align_and_stack(frames, estimator=identity, depth_map=0.0, depth_refine=REFINE, stereo=sv, depth_composite=dc,
                                      info=info, arith="exact")
    img0, _ = pipeline.align_and_stack(frames, estimator=identity, depth_map=0.0, stereo=sv, depth_composite=dc, info=plain,
                                       arith="exact")
    assert np.array_equal(img, img0)
    # by hand: the handle's own map, energy and fused frame
    st = L.Stack(64, 96, in_dtype=np.uint8, arith="exact")
    try:
        for f in pushed:
            st.push_frame(f)
        fused = st.finish()
        assert np.array_equal(fused, img)
        want = gr.guided_refine(st.depth_map(0.0), st.tap(L.TAP_ENERGY, 0), fused, 6, 1e-4, 0, n - 1)
        assert np.array_equal(plain["depth_map"], st.depth_map(0.0))
    finally:
        st.close()
    assert np.array_equal(info["depth_map"], want) and not np.array_equal(want, plain["depth_map"])
    assert np.array_equal(info["stereo"], stereo.pair(img, want, n, 3.0, 0.5, "last", "parallel"))
    assert np.array_equal(info["depth_composite"], depth_render.composite(pushed, want, "linear"))
    assert not np.array_equal(info["depth_composite"], plain["depth_composite"])
    # depth_refine=None is the call without the argument
    none = {}
    img1, _ = pipeline.align_and_stack(frames, estimator=identity, depth_map=0.0, depth_refine=None, stereo=sv, depth_composite=dc,
                                       info=none, arith="exact")
    assert np.array_equal(img1, img0) and all(np.array_equal(none[k], plain[k]) for k in ("depth_map", "stereo", "depth_composite"))
    # the guide is the fused frame before the post-stack filters: the map does not move with them
    filt = {}
    pipeline.align_and_stack(frames, estimator=identity, depth_map=0.0, depth_refine=REFINE, info=filt, arith="exact",
                             unsharp=(2.0, 1.0, 0.0), white_balance=(1.2, 1.0, 0.8))
    assert np.array_equal(filt["depth_map"], want)
    for bad in (dict(depth_refine=REFINE), dict(depth_refine={"radius": 0}, depth_map=0.0), dict(depth_refine={"size": 3}, depth_map=0.0)):
        with pytest.raises(InvalidOptionError):
            pipeline.align_and_stack(frames, estimator=identity, info={}, **bad)
    with pytest.raises(InvalidOptionError):
        pipeline.bunches_then_stack(lambda i: frames[i], n, 64, 96, np.uint8, depth_refine=REFINE)


def test_align_and_stack_device_refines_every_depth_map(L):
    from shinestacker_amd import depth_render, pipeline, stereo
    n, h, w = 8, 96, 160
    fb = h * w * 3
    frames, out_dev = L.DeviceBuffer(n * fb), L.DeviceBuffer(fb)
    handles = None
    try:
        L.synth_frames_device(frames.ptr, np.uint8, h, w, 0, n, n)
        sv, dc = {"layout": "anaglyph"}, {"interp": "nearest"}
        info, plain, none = {}, {}, {}
        img, tr, cc, handles = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, depth_map=0.0, depth_refine=REFINE, stereo=sv,
                                                               depth_composite=dc, info=info, keep_handles=True)
        st = handles.stack
        want = gr.guided_refine(st.depth_map(0.0), st.tap(L.TAP_ENERGY, 0), img, 6, 1e-4, 0, n - 1)
        assert np.array_equal(info["depth_map"], want) and not np.array_equal(want, st.depth_map(0.0))
        assert np.array_equal(info["stereo"], stereo.pair(img, want, n, stereo.DEFAULT_SEPARATION, 0.5, "last", "anaglyph"))
        aligned = list(handles.batches.download((n, h, w, 3), np.uint8))
        comp = info["depth_composite"]
        try:
            assert np.array_equal(comp.download((h, w, 3), np.uint8), depth_render.composite(aligned, want, "nearest"))
        finally:
            comp.free()
        img0, tr0, cc0 = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, depth_map=0.0, stereo=sv, info=plain)
        img1, tr1, cc1 = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, depth_map=0.0, stereo=sv, info=none,
                                                         depth_refine=None)
        assert np.array_equal(img, img0) and np.array_equal(img1, img0) and cc0 == cc1 == cc
        assert np.array_equal(none["depth_map"], plain["depth_map"]) and np.array_equal(none["stereo"], plain["stereo"])
        # with out_dev the refined map stays on the device
        dev = {}
        res = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, depth_map=0.0, depth_refine=REFINE, info=dev, out_dev=out_dev.ptr)
        assert res[0] is None
        try:
            assert np.array_equal(dev["depth_map"].download((h, w), np.float32), want)
        finally:
            dev["depth_map"].free()
    finally:
        if handles is not None:
            pipeline.close_handles(handles)
        frames.free()
        out_dev.free()


def test_focus_stack_writes_the_refined_depth_map(L, tmp_path):
    import shutil
    from shinestacker_amd import FocusStack, InvalidOptionError, PyramidStack, StackJob, depth_out
    from shinestacker_amd.imageio import read_img
    work = tmp_path / "job"
    (work / "src").mkdir(parents=True)
    for fn in sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop"))):
        shutil.copy(os.path.join(GOLDEN, "img_jpg_crop", fn), work / "src" / fn)
    algo = PyramidStack()
    try:
        job = StackJob("job", str(work), input_path="src")
        job.add_action(FocusStack("stack", algo, depth_map_path="depth", depth_map_sigma=0.0, depth_refine=REFINE))
        job.run()
        back = read_img(str(work / "depth" / "stack_0000.png"))
        back = back[:, :, 0] if back.ndim == 3 else back
        refined = algo.depth_map(0.0, refine=REFINE)
        assert back.dtype == np.uint16 and np.array_equal(back, depth_out.quantize(refined, 6))
        assert not np.array_equal(back, depth_out.quantize(algo.depth_map(0.0), 6))
        fused = read_img(str(work / "stack" / "stack_0000.png"))
        en = algo._stack.tap(L.TAP_ENERGY, 0)
        assert np.array_equal(refined, gr.guided_refine(algo.depth_map(0.0), en, fused, 6, 1e-4, 0, 5))
        with pytest.raises(InvalidOptionError):
            FocusStack("none", algo, depth_refine=REFINE)               # nothing asks for a depth map
        with pytest.raises(InvalidOptionError):
            FocusStack("bad", algo, depth_map_path="depth", depth_refine={"radius": 99})
    finally:
        algo.close()
