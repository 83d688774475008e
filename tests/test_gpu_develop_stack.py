"""GPU: development on the mosaic upload path of a stack handle (csrc/mosaic_host.hpp).  Frames pushed with
push_mosaic(m, cfa, develop) must fuse exactly as the same frames developed one by one with debayer(m, cfa, develop) and pushed
as BGR: the fused image and the level-0 winner-index tap are array_equal.  Ten frames with batch_frames = 4 -- two full batches
and a tail of two -- at the shapes of test_gpu_mosaic_stack.py.  The development itself is held to its restatement by
test_gpu_develop.py; here `debayer` is the reference."""
import numpy as np
import pytest

from test_gpu_mosaic_stack import CASES, N, make_mosaics

pytestmark = pytest.mark.gpu

CAMERA = [[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [0.05, -0.55, 1.5]]


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


@pytest.fixture(scope="module")
def data(dev):
    """per case: (cfa, develop, mosaics, plain frames, developed frames) -- twelve frames, the stack tests use the first ten"""
    from shinestacker_amd import Cfa, Develop, debayer
    d = {}
    for name, (h, w, dtype, pattern) in CASES.items():
        mx = int(np.iinfo(dtype).max)
        cfa = Cfa(pattern, black=mx // 64, gains=[1.8, 1.0, 1.0, 1.4])
        mosaics = make_mosaics(h, w, dtype, 12, seed=h)
        mask = np.random.default_rng(w).random((h, w)) < 0.01
        hot = []
        for m in mosaics:            # the sensor's defects: hot sites, the same in every frame
            m = m.copy()
            m[mask] = mx
            hot.append(m)
        develop = Develop(matrix=CAMERA, tone="srgb", defects=mask)
        plain = [debayer(m, cfa) for m in hot]
        developed = [debayer(m, cfa, develop) for m in hot]
        assert not np.array_equal(plain[0], developed[0])
        d[name] = (cfa, develop, hot, plain, developed)
    yield d
    for v in d.values():
        v[1].close()


def run(lib, st, cfa, develop, mosaics, plain, developed, kinds, zero_copy=False):
    """push frame k as a developed mosaic ('d'), a plain mosaic ('m'), its developed BGR frame ('D') or its plain BGR frame ('f');
    (fused image, level-0 winner indices)"""
    keep = []
    for k, kind in enumerate(kinds):
        src = {"d": mosaics, "m": mosaics, "D": developed, "f": plain}[kind][k]
        if zero_copy:
            pinned = lib.host_alloc(src.shape, src.dtype)
            pinned[...] = src
            keep.append(pinned)
            src = pinned
        if kind == "d":
            st.push_mosaic(src, cfa, zero_copy=zero_copy, develop=develop)
        elif kind == "m":
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


@pytest.mark.parametrize("zero_copy", [False, True], ids=["pageable", "zero_copy"])
@pytest.mark.parametrize("case", list(CASES))
def test_developed_mosaics_fuse_as_their_developed_frames(dev, data, case, zero_copy):
    cfa, develop, mosaics, plain, developed = data[case]
    args = (cfa, develop, mosaics[:N], plain[:N], developed[:N])
    with new_stack(dev, case) as st:
        want, want_idx = run(dev, st, *args, "D" * N)
        assert len(np.unique(want_idx)) > 3          # the winners come from many frames: order and batching matter
        st.reset()
        got, got_idx = run(dev, st, *args, "d" * N, zero_copy=zero_copy)
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)
        assert not st._develops                      # finish let go of the Develop
        st.reset()
        again, again_idx = run(dev, st, *args, "d" * N, zero_copy=zero_copy)
        assert np.array_equal(again_idx, want_idx) and np.array_equal(again, want)
        # developed mosaics and developed BGR frames alternating, in runs that end inside a batch
        for kinds in ("dD" * (N // 2), "dddDDddddD"):
            st.reset()
            mixed, mixed_idx = run(dev, st, *args, kinds, zero_copy=zero_copy)
            assert np.array_equal(mixed_idx, want_idx) and np.array_equal(mixed, want), kinds
    # a handle that only ever saw developed mosaics
    with new_stack(dev, case) as st:
        got, got_idx = run(dev, st, *args, "d" * N, zero_copy=zero_copy)
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)


@pytest.mark.parametrize("case", list(CASES))
def test_plain_developed_and_bgr_pushes_interleave(dev, data, case):
    """frame by frame on one handle: plain mosaics, developed mosaics and BGR frames of both kinds"""
    cfa, develop, mosaics, plain, developed = data[case]
    args = (cfa, develop, mosaics[:N], plain[:N], developed[:N])
    with new_stack(dev, case) as st:
        for kinds, same in (("mdfDmdfDmd", "fDfDfDfDfD"), ("ddmmmdDfdm", "DDfffDDfDf")):
            want, want_idx = run(dev, st, *args, same)
            st.reset()
            got, got_idx = run(dev, st, *args, kinds)
            st.reset()
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want), kinds
        # a plain push after developed ones is the plain demosaic again
        want, want_idx = run(dev, st, *args, "f" * N)
        st.reset()
        st.push_mosaic(mosaics[0], cfa, develop=develop)
        st.reset()
        got, got_idx = run(dev, st, *args, "m" * N)
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("how", ["simple", "f64"])
def test_synchronous_routes(dev, data, how, case):
    """MI_IMPL_SIMPLE and float-64 handles: upload, defects, developed demosaic, push, wait"""
    cfa, develop, mosaics, plain, developed = data[case]
    args = (cfa, develop, mosaics[:4], plain[:4], developed[:4])
    kw = dict(impl=dev.IMPL_SIMPLE) if how == "simple" else dict(float_type=dev.MI_F64)
    with new_stack(dev, case, **kw) as st:
        want, want_idx = run(dev, st, *args, "DDDD")
        for kinds in ("dddd", "dDdD"):
            st.reset()
            got, got_idx = run(dev, st, *args, kinds)
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want), kinds
        st.reset()
        want, want_idx = run(dev, st, *args, "fDfD")
        st.reset()
        got, got_idx = run(dev, st, *args, "mdmd")
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got, want)


def test_push_rejects_misuse_and_keeps_its_develops(dev, data):
    from shinestacker_amd import Develop, InvalidOptionError
    from shinestacker_amd.errors import BitDepthError
    cfa, develop, mosaics, plain, developed = data["u8"]
    with new_stack(dev, "u8") as st:
        with pytest.raises(InvalidOptionError):
            st.push_mosaic(mosaics[0], cfa, develop="srgb")
        with pytest.raises(BitDepthError):
            st.push_mosaic(mosaics[0], cfa, develop=Develop(tone=np.arange(65536).astype(np.uint16)))
        with pytest.raises(InvalidOptionError):
            st.push_mosaic(mosaics[0], cfa, develop=Develop(defects=np.zeros((3, 3), bool)))
        assert st.frames_pushed == 0 and not st._develops
        other = Develop(tone=2.2)
        st.push_mosaic(mosaics[0], cfa, develop=develop)
        st.push_mosaic(mosaics[1], cfa, develop=other)
        st.push_mosaic(mosaics[2], cfa, develop=develop)
        assert len(st._develops) == 2 and st._develops[0] is develop and st._develops[1] is other
        st.reset()
        assert not st._develops
        other.close()


@pytest.mark.parametrize("case", list(CASES))
def test_focus_stack_arrays_develops_mosaics(dev, data, case):
    from shinestacker_amd import PyramidStack
    cfa, develop, mosaics, plain, developed = data[case]
    algo = PyramidStack(batch_frames=4)
    try:
        want = algo.focus_stack_arrays(developed[:N])
        got = algo.focus_stack_arrays(mosaics[:N], mosaic=cfa, develop=develop)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert not np.array_equal(got, algo.focus_stack_arrays(mosaics[:N], mosaic=cfa))
    finally:
        algo.close()


def test_bunches_then_stack_develops_mosaics(dev, data):
    from shinestacker_amd import pipeline
    cfa, develop, mosaics, plain, developed = data["u16"]
    h, w, dtype, _ = CASES["u16"]
    taps = {"f": [], "m": []}
    want, bunches = pipeline.bunches_then_stack(lambda i: developed[i], 12, h, w, dtype, frames=5, overlap=2, batch_frames=4,
                                                on_final=lambda st, buf: taps["f"].append(st.tap(dev.TAP_INDEX, 0)))
    got, bunches_m = pipeline.bunches_then_stack(lambda i: mosaics[i], 12, h, w, dtype, frames=5, overlap=2, batch_frames=4, mosaic=cfa,
                                                 develop=develop, on_final=lambda st, buf: taps["m"].append(st.tap(dev.TAP_INDEX, 0)))
    assert bunches == bunches_m and len(bunches) > 2
    assert np.array_equal(taps["m"][0], taps["f"][0]) and np.array_equal(got, want)
