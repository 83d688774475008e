"""GPU: the depth map output (csrc/kernels_depth.hpp) against its NumPy restatement (tests/depth_restatement.py), bit for bit:
the stand-alone smoothing primitive on crafted planes, PyramidStack.depth_map against the oracle's recorded level-0 state and
against the handle's own taps, DepthMapStack.depth_map against its taps, and the options of the actions and the pipeline."""
import os

import numpy as np
import pytest

import depth_restatement as dr
from conftest import GOLDEN, load_golden, stack_kwargs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


def planes(shape, seed, dtype=np.float32, vmax=12, wmax=50.0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, vmax + 1, shape).astype(np.int32), (rng.random(shape) * wmax).astype(dtype)


# ------------------------------------------------------------------ the primitive
# 5 x 7: smaller than any tile; 37 x 53: ragged both ways; 131 x 197: several column tiles (64 x 32) and, at sigma 16, a halo
# of 48 that is wider than a tile side; 300 x 70 / 40 x 600: more than one 256-pixel row segment, more than 8 row groups
@pytest.mark.parametrize("shape,sigma", [((5, 7), 0.5), ((37, 53), 2.0), ((131, 197), 2.0), ((131, 197), 16.0), ((131, 197), 0.0),
                                         ((49, 49), 16.0), ((40, 600), 1.0), ((300, 70), 3.0)])
def test_weighted_smooth_float32(L, shape, sigma):
    from shinestacker_amd import depth_out
    v, w = planes(shape, 1 + shape[0])
    got = depth_out.weighted_smooth(v, w, sigma)
    assert got.dtype == np.float32 and got.shape == shape
    assert np.array_equal(got, dr.weighted_smooth(v, w, sigma, np.float32))
    if sigma > 0:   # a float value plane takes the same path
        vf = (v.astype(np.float32) + np.float32(0.25))
        assert np.array_equal(depth_out.weighted_smooth(vf, w, sigma), dr.weighted_smooth(vf, w, sigma, np.float32))


@pytest.mark.parametrize("shape,sigma", [((37, 53), 2.0), ((37, 53), 0.0), ((70, 300), 4.0)])
def test_weighted_smooth_float64(L, shape, sigma):
    from shinestacker_amd import depth_out
    v, w = planes(shape, 3, np.float64)
    assert np.array_equal(depth_out.weighted_smooth(v, w, sigma), dr.weighted_smooth(v, w, sigma, np.float64))
    vd = v.astype(np.float64) + 0.125
    assert np.array_equal(depth_out.weighted_smooth(vd, w, sigma), dr.weighted_smooth(vd, w, sigma, np.float64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weighted_smooth_contents(L, dtype):
    from shinestacker_amd import depth_out
    shape, sigma = (90, 117), 2.0      # radius 6: a window of 13
    rng = np.random.default_rng(17)
    # patches of zero weight larger than the window: the fallback to v, next to pixels that do divide
    v, w = planes(shape, 19, dtype)
    w[10:40, 20:60] = 0
    w[70:, :30] = 0
    w[:20, 100:] = 0
    got = depth_out.weighted_smooth(v, w, sigma)
    assert np.array_equal(got, dr.weighted_smooth(v, w, sigma, dtype))
    assert np.array_equal(got[17:33, 27:53], v[17:33, 27:53].astype(np.float32))     # whole window inside the first patch
    # no weight anywhere: the values themselves
    zero = np.zeros(shape, dtype)
    assert np.array_equal(depth_out.weighted_smooth(v, zero, sigma), v.astype(np.float32))
    # indices up to 255 with energies up to 4.3e9 (the uint16 range: 65535^2)
    v = rng.integers(0, 256, shape).astype(np.int32)
    w = (rng.random(shape) ** 4 * 4.3e9).astype(dtype)
    got = depth_out.weighted_smooth(v, w, sigma)
    assert np.array_equal(got, dr.weighted_smooth(v, w, sigma, dtype))
    assert got.min() >= 0 and got.max() <= 255.001


# ------------------------------------------------------------------ PyramidStack
@pytest.mark.parametrize("case", ["g1_u8", "g2_u16"])
def test_pyramid_depth_map_against_the_oracle_state(L, case):
    """arith='exact' is bit-identical to the oracle, whose level-0 energy and arg-max for these frames are in the fixture"""
    from shinestacker_amd import PyramidStack
    g = load_golden(case)
    algo = PyramidStack(arith="exact", **stack_kwargs(g["params"]))
    try:
        out = algo.focus_stack_arrays(list(g["frames"]))
        assert np.array_equal(out, g["final"])
        idx, en = g["best_0"].astype(np.int32), g["energy_0"]
        for sigma in (0.0, 2.0):
            got = algo.depth_map(sigma)
            assert got.dtype == np.float32 and got.shape == idx.shape
            assert np.array_equal(got, dr.weighted_smooth(idx, en, sigma, np.float32)), sigma
        assert np.array_equal(algo.depth_map(), algo.depth_map(2.0))          # the default
        assert got.min() >= 0 and got.max() <= len(g["frames"]) - 1 + 1e-3
    finally:
        algo.close()


@pytest.mark.parametrize("arith,float_type,impl", [("exact", "f32", 1), ("exact", "f32", 2), ("separable", "f32", 1),
                                                   ("separable", "f32", 0), ("exact", "f64", 0)])
def test_pyramid_depth_map_against_its_own_taps_and_leaves_the_state_alone(L, arith, float_type, impl):
    g = load_golden("g1_u8")
    fr = g["frames"]
    f64 = float_type == "f64"
    st = L.Stack(fr.shape[1], fr.shape[2], in_dtype=fr.dtype, arith=arith, impl=impl, float_type=L.MI_F64 if f64 else L.MI_F32,
                 **stack_kwargs(g["params"]))
    try:
        for f in fr:
            st.push_frame(f)
        idx, en = st.tap(L.TAP_INDEX, 0), st.tap(L.TAP_ENERGY, 0)
        dt = np.float64 if f64 else np.float32
        first = st.depth_map(2.0)
        assert np.array_equal(first, dr.weighted_smooth(idx, en, 2.0, dt))
        assert np.array_equal(st.depth_map(0.0), idx.astype(np.float32))
        assert np.array_equal(st.depth_map(16.0), dr.weighted_smooth(idx, en, 16.0, dt))
        # a second call and the state behind it are unchanged, and so is what finish makes of that state
        assert np.array_equal(st.depth_map(2.0), first)
        assert np.array_equal(st.tap(L.TAP_INDEX, 0), idx) and np.array_equal(st.tap(L.TAP_ENERGY, 0), en)
        out = st.finish()
        ref = L.Stack(fr.shape[1], fr.shape[2], in_dtype=fr.dtype, arith=arith, impl=impl,
                      float_type=L.MI_F64 if f64 else L.MI_F32, **stack_kwargs(g["params"]))
        try:
            for f in fr:
                ref.push_frame(f)
            assert np.array_equal(out, ref.finish())
            assert np.array_equal(st.tap(L.TAP_FUSED_LAP, 0), ref.tap(L.TAP_FUSED_LAP, 0))
        finally:
            ref.close()
        assert np.array_equal(st.depth_map(2.0), first)      # after finish as before it
        # into device memory
        buf = L.DeviceBuffer(first.nbytes)
        try:
            assert st.depth_map(2.0, buf.ptr) is None
            assert np.array_equal(buf.download(first.shape, np.float32), first)
        finally:
            buf.free()
    finally:
        st.close()


def test_pyramid_depth_map_reports_global_indices(L):
    g = load_golden("g1_u8")
    fr = g["frames"]
    kw = stack_kwargs(g["params"])
    plain = L.Stack(fr.shape[1], fr.shape[2], in_dtype=fr.dtype, **kw)
    shard = L.Stack(fr.shape[1], fr.shape[2], in_dtype=fr.dtype, **kw)
    try:
        shard.set_first_index(3, stride=2)
        for f in fr:
            plain.push_frame(f)
            shard.push_frame(f)
        k, en = plain.tap(L.TAP_INDEX, 0), plain.tap(L.TAP_ENERGY, 0)
        glob = (3 + 2 * k).astype(np.int32)
        # before the indices are exported (the handle still holds its consecutive numbering) ...
        assert np.array_equal(shard.depth_map(0.0), glob.astype(np.float32))
        assert np.array_equal(shard.depth_map(2.0), dr.weighted_smooth(glob, en, 2.0, np.float32))
        # ... and after (the tap exports them in place)
        assert np.array_equal(shard.tap(L.TAP_INDEX, 0), glob)
        assert np.array_equal(shard.depth_map(0.0), glob.astype(np.float32))
        assert np.array_equal(shard.depth_map(2.0), dr.weighted_smooth(glob, en, 2.0, np.float32))
    finally:
        plain.close()
        shard.close()


def test_pyramid_depth_map_call_order_and_options(L):
    from shinestacker_amd import InvalidOptionError, PyramidStack
    algo = PyramidStack(min_size=16)      # one Laplacian level at 40 x 48
    with pytest.raises(RuntimeError):
        algo.depth_map()
    st = L.Stack(64, 80)
    try:
        with pytest.raises(RuntimeError):       # MI_ERR_STATE: nothing pushed
            st.depth_map(1.0)
        st.push_frame(np.zeros((64, 80, 3), np.uint8))
        with pytest.raises(ValueError):         # MI_ERR_INVALID from the library itself
            st.depth_map(17.0)
        with pytest.raises(ValueError):
            st.depth_map(-1.0)
    finally:
        st.close()
    algo.focus_stack_arrays([np.zeros((40, 48, 3), np.uint8)] * 2)
    try:
        with pytest.raises(InvalidOptionError):
            algo.depth_map(14.0)                # radius 42 >= 40
        assert np.array_equal(algo.depth_map(1.0), np.zeros((40, 48), np.float32))   # flat frames: the first frame wins
    finally:
        algo.close()


# ------------------------------------------------------------------ DepthMapStack
DM_CASES = [("dm_default_u8", {}),                                                      # AVERAGE, smoothed, float-32
            ("dm_max_u8", {"map_type": "max"}),                                         # MAX, smoothed
            ("dm_nosmooth_k3_u8", {"smooth_size": 0, "kernel_size": 3, "blur_size": 3}),   # AVERAGE, smooth_size 0
            ("dm_f64_default_u8", {"float_type": "float-64"}),                          # float-64, float32 planes
            ("dm_f64_max_nosmooth_u16", {"float_type": "float-64", "map_type": "max", "smooth_size": 0, "blur_size": 9})]  # W = float64


@pytest.mark.parametrize("name,kw", DM_CASES)
def test_depth_map_stack_depth_map(L, name, kw):
    from shinestacker_amd import DepthMapStack
    g = load_golden("depth_map")
    frames = list(g[name + "_frames"])
    dms = DepthMapStack(**kw)
    try:
        out = dms.focus_stack_arrays(frames)
        h = dms._dmap
        ins = np.stack([h.tap(L.DM_TAP_ENERGY_IN, i) for i in range(len(frames))])
        tot = h.tap(L.DM_TAP_TOTAL)
        wide = kw.get("float_type") == "float-64" and kw.get("smooth_size", 15) == 0
        assert ins.dtype == (np.float64 if wide else np.float32)
        average = kw.get("map_type", "average") == "average"
        for sigma in (0.0, 2.0):
            got = dms.depth_map(sigma)
            assert got.dtype == np.float32 and got.shape == tot.shape
            assert np.array_equal(got, dr.depth_map_stack(ins, tot, sigma, average)), (name, sigma)
            assert got.min() >= 0 and got.max() <= len(frames) - 1 + 1e-3
        assert np.array_equal(dms.depth_map(), dms.depth_map(0.0))      # the default
        # the state is read only
        assert np.array_equal(np.stack([h.tap(L.DM_TAP_ENERGY_IN, i) for i in range(len(frames))]), ins)
        assert np.array_equal(h.tap(L.DM_TAP_TOTAL), tot)
        buf = L.DeviceBuffer(got.nbytes)
        try:
            assert dms.depth_map(2.0, buf.ptr) is None
            assert np.array_equal(buf.download(got.shape, np.float32), got)
        finally:
            buf.free()
        assert np.array_equal(out, DepthMapStack(**kw).focus_stack_arrays(frames))
    finally:
        dms.close()


def test_depth_map_stack_before_finish(L):
    from shinestacker_amd import DepthMapStack, DeviceError
    with pytest.raises(RuntimeError):
        DepthMapStack().depth_map()
    d = L.DepthMap(40, 48)
    try:
        d.push_frame(np.random.default_rng(2).integers(0, 256, (40, 48, 3)).astype(np.uint8))
        with pytest.raises(DeviceError):            # MI_ERR_STATE, the binding's usual exception
            d.depth_map(0.0)
        assert L.load().mi_dmap_depth_map(d._h, 0.0, np.empty((40, 48), np.float32).ctypes.data) == L.MI_ERR_STATE
        d.finish()
        got = d.depth_map(0.0)                      # one frame: every defined weight is on frame 0
        assert got.shape == (40, 48) and got.dtype == np.float32 and np.array_equal(got, np.zeros((40, 48), np.float32))
    finally:
        d.close()


# ------------------------------------------------------------------ actions and pipeline
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


def test_focus_stack_writes_the_depth_map(L, tmp_path):
    from shinestacker_amd import depth_out
    from shinestacker_amd.imageio import read_img
    work, algo = _run_focus_stack(tmp_path, "with", depth_map_path="depth")
    try:
        png = work / "depth" / "stack_0000.png"
        assert png.is_file()
        back = read_img(str(png))
        back = back[:, :, 0] if back.ndim == 3 else back
        want = depth_out.quantize(algo.depth_map(), 6)
        assert back.dtype == np.uint16 and np.array_equal(back, want)
        assert want.max() > want.min()                       # six frames focused at different depths: not a flat map
        stacked = read_img(str(work / "stack" / "stack_0000.png"))
    finally:
        algo.close()
    plain, algo2 = _run_focus_stack(tmp_path, "without")
    algo2.close()
    assert not (plain / "depth").exists()
    assert np.array_equal(stacked, read_img(str(plain / "stack" / "stack_0000.png")))
    # an explicit sigma
    work0, algo0 = _run_focus_stack(tmp_path, "sigma0", depth_map_path="depth", depth_map_sigma=0.0)
    try:
        back = read_img(str(work0 / "depth" / "stack_0000.png"))
        back = back[:, :, 0] if back.ndim == 3 else back
        assert np.array_equal(back, depth_out.quantize(algo0.depth_map(0.0), 6))
    finally:
        algo0.close()


def test_align_and_stack_device_returns_the_depth_map(L):
    from shinestacker_amd import pipeline
    n, h, w = 8, 96, 160
    fb = h * w * 3
    frames = L.DeviceBuffer(n * fb)
    out_a, out_b = L.DeviceBuffer(fb), L.DeviceBuffer(fb)
    handles = None
    try:
        L.synth_frames_device(frames.ptr, np.uint8, h, w, 0, n, n)
        info = {}
        img, tr, cc, handles = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, depth_map=2.0, info=info,
                                                               keep_handles=True)
        assert isinstance(info["depth_map"], np.ndarray) and info["depth_map"].dtype == np.float32
        assert np.array_equal(info["depth_map"], handles.stack.depth_map(2.0))
        assert info["depth_map"].shape == (h, w) and 0 <= info["depth_map"].min() and info["depth_map"].max() <= n - 1 + 1e-3
        img0, tr0, cc0 = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8)
        assert np.array_equal(img, img0) and cc == cc0
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(tr, tr0))
        # with out_dev the map stays on the device as well; True is the default sigma
        info_d = {}
        res = pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, depth_map=True, info=info_d, out_dev=out_a.ptr)
        assert res[0] is None
        try:
            assert np.array_equal(info_d["depth_map"].download((h, w), np.float32), info["depth_map"])
        finally:
            info_d["depth_map"].free()
        assert np.array_equal(out_a.download((h, w, 3), np.uint8), img)
        # off: nothing is added
        info_n = {}
        pipeline.align_and_stack_device(frames.ptr, n, h, w, np.uint8, info=info_n, out_dev=out_b.ptr)
        assert "depth_map" not in info_n
    finally:
        if handles is not None:
            pipeline.close_handles(handles)
        for b in (frames, out_a, out_b):
            b.free()


def test_align_and_stack_returns_the_depth_map(L):
    from shinestacker_amd import pipeline
    n, h, w = 4, 96, 160
    dev = L.DeviceBuffer(n * h * w * 3)
    try:
        L.synth_frames_device(dev.ptr, np.uint8, h, w, 0, n, n)
        frames = list(dev.download((n, h, w, 3), np.uint8))
    finally:
        dev.free()

    def identity(a, b, *_cfg):
        return 100, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    info = {}
    img, _ = pipeline.align_and_stack(frames, estimator=identity, depth_map=True, info=info)
    img0, _ = pipeline.align_and_stack(frames, estimator=identity)
    assert np.array_equal(img, img0)
    d = info["depth_map"]
    assert d.dtype == np.float32 and d.shape == (h, w) and 0 <= d.min() and d.max() <= n - 1 + 1e-3
