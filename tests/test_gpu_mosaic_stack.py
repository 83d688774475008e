"""GPU: the mosaic upload path of a stack handle (csrc/mosaic_host.hpp).  Frames pushed as raw mosaics must fuse exactly as the
same frames demosaiced first and pushed as BGR: the fused image and the level-0 winner-index tap are array_equal.  Ten frames
with batch_frames = 4 -- two full batches and a tail of two -- of 130 x 170 uint16 and 131 x 171 uint8.  The demosaic itself is
held to its restatement by test_gpu_demosaic.py; here `debayer` is the reference."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 10
CASES = {"u16": (130, 170, np.uint16, "RGGB"), "u8": (131, 171, np.uint8, "GBRG")}


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


def make_mosaics(h, w, dtype, n, seed):
    """n mosaics of a scene whose focus moves across the frame: detail (noise) in a band that differs per frame, smooth elsewhere"""
    rng = np.random.default_rng(seed)
    mx = int(np.iinfo(dtype).max)
    y, x = np.mgrid[0:h, 0:w]
    smooth = (0.5 + 0.3 * np.sin(x / 23.0) * np.cos(y / 17.0)) * mx
    detail = rng.integers(-mx // 3, mx // 3, size=(h, w))
    out = []
    for i in range(n):
        centre = (i + 0.5) * w / n
        sharp = np.exp(-((x - centre) / (0.8 * w / n)) ** 2)
        noise = rng.integers(-mx // 100 - 1, mx // 100 + 2, size=(h, w))
        out.append(np.clip(smooth + sharp * detail + noise, 0, mx).astype(dtype))
    return out


@pytest.fixture(scope="module")
def data(dev):
    """per case: (cfa, mosaics, their debayered frames) -- twelve frames, the stack tests use the first ten"""
    from shinestacker_amd import Cfa, debayer
    d = {}
    for name, (h, w, dtype, pattern) in CASES.items():
        mx = int(np.iinfo(dtype).max)
        cfa = Cfa(pattern, black=mx // 64, gains=[1.8, 1.0, 1.0, 1.4])
        mosaics = make_mosaics(h, w, dtype, 12, seed=h)
        d[name] = (cfa, mosaics, [debayer(m, cfa) for m in mosaics])
    return d


def run(lib, st, cfa, mosaics, frames, kinds, zero_copy=False):
    """push frame k as a mosaic ('m') or as its debayered BGR frame ('f'); (fused image, level-0 winner indices)"""
    keep = []
    for k, kind in enumerate(kinds):
        src = mosaics[k] if kind == "m" else frames[k]
        if zero_copy:
            pinned = lib.host_alloc(src.shape, src.dtype)
            pinned[...] = src
            keep.append(pinned)
            src = pinned
        if kind == "m":
            st.push_mosaic(src, cfa, zero_copy=zero_copy)
        else:
            st.push_frame(src, zero_copy=zero_copy)
        assert st.frames_pushed == k + 1
    if zero_copy:
        st.wait_uploads(0)
    idx = st.tap(lib.TAP_INDEX, 0)
    return st.finish(), idx


def new_stack(lib, case, **kw):
    h, w, dtype, _ = CASES[case]
    return lib.Stack(h, w, in_dtype=dtype, batch_frames=4, **kw)


@pytest.mark.parametrize("arith", ["exact", "separable"])
@pytest.mark.parametrize("case", list(CASES))
def test_mosaics_fuse_as_their_debayered_frames(dev, data, case, arith):
    cfa, mosaics, frames = data[case]
    mosaics, frames = mosaics[:N], frames[:N]
    with new_stack(dev, case, arith=arith) as st:
        want, want_idx = run(dev, st, cfa, mosaics, frames, "f" * N)
        assert len(np.unique(want_idx)) > 3          # the winners come from many frames: order and batching matter
        st.reset()
        got, got_idx = run(dev, st, cfa, mosaics, frames, "m" * N)
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)
        # after a reset the same handle gives the same result again
        st.reset()
        assert st.frames_pushed == 0
        again, again_idx = run(dev, st, cfa, mosaics, frames, "m" * N)
        assert np.array_equal(again_idx, want_idx) and np.array_equal(again, want)
        # both kinds alternating, and in runs that end inside a batch: call order is frame order
        for kinds in ("fm" * (N // 2), "mf" * (N // 2), "mmmffmmmmf"):
            st.reset()
            mixed, mixed_idx = run(dev, st, cfa, mosaics, frames, kinds)
            assert np.array_equal(mixed_idx, want_idx) and np.array_equal(mixed, want), kinds
    # a handle that only ever saw mosaics
    with new_stack(dev, case, arith=arith) as st:
        got, got_idx = run(dev, st, cfa, mosaics, frames, "m" * N)
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)


@pytest.mark.parametrize("case", list(CASES))
def test_order_survives_batching(dev, data, case):
    """frames 3 and 7 are identical and the sharpest somewhere: the first maximum wins, so no pixel may name 7"""
    cfa, mosaics, frames = data[case]
    mosaics, frames = list(mosaics[:N]), list(frames[:N])
    mosaics[7], frames[7] = mosaics[3], frames[3]
    with new_stack(dev, case) as st:
        want, want_idx = run(dev, st, cfa, mosaics, frames, "f" * N)
        assert (want_idx == 3).any() and not (want_idx == 7).any()
        for kinds in ("m" * N, "fm" * (N // 2)):
            st.reset()
            got, got_idx = run(dev, st, cfa, mosaics, frames, kinds)
            assert (got_idx == 3).any() and not (got_idx == 7).any()
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want), kinds


@pytest.mark.parametrize("case", list(CASES))
def test_pinned_and_pageable_routes_agree(dev, data, case):
    cfa, mosaics, frames = data[case]
    mosaics, frames = mosaics[:N], frames[:N]
    with new_stack(dev, case) as st:
        want, want_idx = run(dev, st, cfa, mosaics, frames, "m" * N)
        for kinds in ("m" * N, "mf" * (N // 2)):
            st.reset()
            got, got_idx = run(dev, st, cfa, mosaics, frames, kinds, zero_copy=True)
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want), kinds
        # rows apart: a view with a row stride takes the bounce route
        st.reset()
        h, w = mosaics[0].shape
        wide = [np.zeros((h, w + 5), m.dtype) for m in mosaics]
        for big, m in zip(wide, mosaics):
            big[:, :w] = m
        got, got_idx = run(dev, st, cfa, [big[:, :w] for big in wide], frames, "m" * N)
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)


@pytest.mark.parametrize("how", ["simple", "f64"])
def test_synchronous_routes(dev, data, how):
    """MI_IMPL_SIMPLE and float-64 handles: upload, demosaic, push, wait"""
    cfa, mosaics, frames = data["u16"]
    kw = dict(impl=dev.IMPL_SIMPLE) if how == "simple" else dict(float_type=dev.MI_F64)
    with new_stack(dev, "u16", **kw) as st:
        want, want_idx = run(dev, st, cfa, mosaics[:4], frames[:4], "ffff")
        for kinds in ("mmmm", "mfmf"):
            st.reset()
            got, got_idx = run(dev, st, cfa, mosaics[:4], frames[:4], kinds)
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want), kinds


def test_push_mosaic_rejects_bad_arguments(dev, data):
    from shinestacker_amd import Cfa
    cfa, mosaics, frames = data["u8"]
    with new_stack(dev, "u8") as st:
        with pytest.raises(ValueError):
            st.push_mosaic(frames[0], cfa)                       # a BGR frame is no mosaic
        with pytest.raises(ValueError):
            st.push_mosaic(mosaics[0].astype(np.uint16), cfa)
        with pytest.raises(Exception):
            st.push_mosaic(mosaics[0], Cfa(white=256))           # above uint8's maximum
        assert st.frames_pushed == 0
    with dev.Stack(64, 64, in_dtype=np.float32) as st:
        c = cfa.struct(np.uint8)
        import ctypes
        rc = dev.load().mi_stack_push_mosaic(st._h, mosaics[0].ctypes.data, 0, ctypes.byref(c), 0)
        assert rc == dev.MI_ERR_INVALID and "dtype must be MI_U8 or MI_U16" in dev.last_error()


@pytest.mark.parametrize("case", list(CASES))
def test_focus_stack_arrays_takes_mosaics(dev, data, case):
    from shinestacker_amd import PyramidStack
    cfa, mosaics, frames = data[case]
    algo = PyramidStack(batch_frames=4)
    try:
        want = algo.focus_stack_arrays(frames[:N])
        got = algo.focus_stack_arrays(mosaics[:N], mosaic=cfa)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    finally:
        algo.close()


def test_bunches_then_stack_takes_mosaics(dev, data):
    from shinestacker_amd import pipeline
    cfa, mosaics, frames = data["u16"]
    h, w, dtype, _ = CASES["u16"]
    taps = {"f": [], "m": []}
    want, bunches = pipeline.bunches_then_stack(lambda i: frames[i], 12, h, w, dtype, frames=5, overlap=2, batch_frames=4,
                                                on_final=lambda st, buf: taps["f"].append(st.tap(dev.TAP_INDEX, 0)))
    got, bunches_m = pipeline.bunches_then_stack(lambda i: mosaics[i], 12, h, w, dtype, frames=5, overlap=2, batch_frames=4, mosaic=cfa,
                                                 on_final=lambda st, buf: taps["m"].append(st.tap(dev.TAP_INDEX, 0)))
    assert bunches == bunches_m and len(bunches) > 2
    assert np.array_equal(taps["m"][0], taps["f"][0]) and np.array_equal(got, want)
