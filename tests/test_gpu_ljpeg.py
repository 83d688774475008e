"""GPU: raw_ljpeg (csrc/kernels_ljpeg.hpp) equals its restatement (tests/ljpeg_restatement.py) bit for bit on the cases of
tests/ljpeg_cases.py -- which the CPU tests show to be meaningful -- in host form and in device form; short streams cost a
status bit and nothing else; a compressed push equals the push of the restated mosaic; and the layers above (dng.develop,
dng.frames_device, PyramidStack(raw=), FocusStack and CombinedActions on folders of compressed .dng files) equal the same call
on the same samples written uncompressed.  Every comparison is array_equal."""
import os

import numpy as np
import pytest

import dng_cases as DC
import ljpeg_cases as LC
import ljpeg_restatement as R
from shinestacker_amd import dng
from shinestacker_amd.errors import ImageLoadError

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of the device buffer the kernel writes


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


@pytest.fixture(scope="module")
def side(dev):
    """a handle whose stream serves as the non-null stream of the device form"""
    st = dev.Stack(64, 64)
    assert st.stream
    yield st
    st.close()


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{case name: (DngFrame, the restated mosaic, the restated status)} of the whole table: written, parsed, restated once"""
    d = tmp_path_factory.mktemp("ljpeg")
    out = {}
    for c in LC.CASES + [s[0] for s in LC.SHORT]:
        c.write(str(d / (c.name + ".dng")))
        frame = dng.read(str(d / (c.name + ".dng")))
        want, status = R.unpack_layout(frame.span, frame.layout)
        want.setflags(write=False)
        out[c.name] = (frame, want, status)
    return out


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def device_form(dev, side, frame, nbytes, stream):
    """(the output between its guard bands, the status words) of raw_ljpeg in device form"""
    up = dng._Staged(frame, 0)
    out = dev.DeviceBuffer(nbytes + 2 * GUARD)
    try:
        out.upload(np.full(out.nbytes, 0xA5, np.uint8))
        up.unpack_into(frame.layout, out.ptr + GUARD, 0, stream)
        if stream:
            side.sync()
        else:
            dev.check(dev.load().mi_device_synchronize(0))
        return out.download((out.nbytes,), np.uint8), up.buf.download((up.nseg,), np.uint32, up.status_at)
    finally:
        out.free()
        up.buf.free()


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_ljpeg_equals_the_restatement(dev, side, table, case):
    """the host form, and the device form between guard bands on the null stream and on a handle's stream; status all zero"""
    frame, want, status = table[case.name]
    assert not status.any() and np.array_equal(want, case.expected())
    assert_same((case, "host"), dng.unpack(frame), want)
    lay, L = frame.layout, frame.layout.struct()
    got = np.empty_like(want)
    st = np.full(len(lay.segments), 0xFFFFFFFF, np.uint32)
    span = dng.host_span(frame)
    dev.check(dev.load().mi_raw_ljpeg(0, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, dev.C.byref(L),
                                      None if lay.table is None else lay.table.ctypes.data, got.ctypes.data, st.ctypes.data))
    assert not st.any()
    assert_same((case, "host, status"), got, want)
    for stream in (None, side.stream):
        raw, st = device_form(dev, side, frame, want.nbytes, stream)
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + want.nbytes:] == 0xA5).all(), "the guard band around the mosaic was written"
        assert not st.any()
        assert_same((case, "device", stream), raw[GUARD:GUARD + want.nbytes].copy().view(want.dtype).reshape(want.shape), want)


@pytest.mark.parametrize("short", LC.SHORT, ids=lambda s: repr(s[0]))
def test_short_streams_cost_a_status_bit_and_nothing_else(dev, side, table, short):
    case, flagged, flag = short
    frame, want, status = table[case.name]
    assert status[flagged] & flag and not np.delete(status, flagged).any()
    _, seg_h, _ = case.segments()
    keep = np.ones(case.h, bool)
    keep[flagged * seg_h:(flagged + 1) * seg_h] = False
    for stream in (None, side.stream):
        raw, st = device_form(dev, side, frame, want.nbytes, stream)
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + want.nbytes:] == 0xA5).all(), "the guard band around the mosaic was written"
        assert st.tolist() == status.tolist()
        got = raw[GUARD:GUARD + want.nbytes].copy().view(want.dtype).reshape(want.shape)
        assert_same((case, "the other segments"), got[keep], want[keep])
    with pytest.raises(ImageLoadError) as e:
        dng.unpack(frame)
    assert frame.path in str(e.value) and f"segment {flagged}" in str(e.value) and f"status {int(status[flagged])}" in str(e.value)


def test_a_span_declared_short_reads_nothing_beyond_it(dev, side, table):
    """bytes at or beyond span_bytes count as 0: the span is DECLARED shorter than the buffer that holds it, so the last strip's
    data ends early -- status bit 1 for that strip, the others exact"""
    frame, want, _ = table["12bit-crop-2-4-strips"]
    lay = frame.layout
    up = dng._Staged(frame, 0)
    out = dev.DeviceBuffer(want.nbytes)
    try:
        last = int(np.argmax(lay.segments["scan_off"]))
        short = int(lay.segments["scan_off"][last]) + int(lay.segments["scan_bytes"][last]) // 2
        dng.unpack_device(lay, up.buf.ptr, short, up.buf.ptr + up.seg_at, None, out.ptr, dev_status=up.status)
        dev.check(dev.load().mi_device_synchronize(0))
        got = out.download(want.shape, want.dtype)
        st = up.buf.download((up.nseg,), np.uint32, up.status_at)
        cut = np.array(frame.span)[:short]
        again, status = R.unpack_layout(cut, lay)
        assert st.tolist() == status.tolist() and status[last] == R.OVERRUN and not np.delete(status, last).any()
        rows = slice(0, last * lay.seg_height - lay.crop_y)
        assert_same("short span", got[rows], want[rows])
    finally:
        out.free()
        up.buf.free()


# ---------------------------------------------------------------------------------------------- stacks
H, W, N = 72, 104, 4
COLOUR = dict(pattern="GRBG", black=(256,), neutral=(0.55, 1.0, 0.7), matrices={1: (DC.XYZ_D65_MATRIX, 21)})


@pytest.fixture(scope="module")
def stack_files(oracle, tmp_path_factory):
    """four 12-bit frames of one synthetic focus stack, each written twice -- lossless JPEG (tiles of 32 x 48 in two
    components, as a converter writes them; strips for the odd frames) and uncompressed -- with one colour description"""
    from shinestacker_amd.demosaic import mosaic_of
    d = tmp_path_factory.mktemp("stack")
    os.makedirs(str(d / "ljpeg"))
    os.makedirs(str(d / "plain"))
    comp, plain, frames, mosaics = [], [], [], []
    for f in range(N):
        bgr = oracle.synth_frame_numpy(H, W, f, N).astype(np.int64)
        stored = mosaic_of(256 + bgr * 15, "GRBG")                    # 12-bit samples over a black level of 256
        p, q = str(d / "ljpeg" / f"f{f:02d}.dng"), str(d / "plain" / f"f{f:02d}.dng")
        geometry = dict(rows_per_strip=7, predictor=1 + f) if f % 2 else dict(tile=(32, 48), predictor=1)
        LC.write_dng(p, stored, 12, ncomp=2, odd_start=True, **geometry, **COLOUR)
        DC.write_dng(q, stored, 12, rows_per_strip=7, **COLOUR)
        comp.append(p)
        plain.append(q)
        frames.append(dng.read(p))
        mosaics.append((stored << 4).astype(np.uint16))
        want, status = R.unpack_layout(frames[-1].span, frames[-1].layout)
        assert not status.any() and np.array_equal(want, mosaics[-1])
    return str(d), comp, plain, frames, mosaics


@pytest.fixture(scope="module")
def bad_file(oracle, tmp_path_factory):
    """frame 0 of the stack in strips of 7 rows, the second strip's stream cut in the middle of its data"""
    from shinestacker_amd.demosaic import mosaic_of
    p = str(tmp_path_factory.mktemp("bad") / "bad.dng")
    stored = mosaic_of(256 + oracle.synth_frame_numpy(H, W, 0, N).astype(np.int64) * 15, "GRBG")
    LC.write_dng(p, stored, 12, ncomp=2, rows_per_strip=7, mangle=LC._cut, **COLOUR)
    return p


@pytest.mark.parametrize("mode", ["separable", "exact", "float-64", "simple"])
def test_push_of_a_compressed_frame_equals_push_mosaic(dev, stack_files, mode):
    """both routes (asynchronous: separable and exact fp32 handles; synchronous: float-64 and MI_IMPL_SIMPLE)"""
    _, _, _, frames, mosaics = stack_files
    kw = dict(in_dtype=np.uint16, min_size=16)
    if mode == "float-64":
        kw.update(float_type=dev.MI_F64, arith="exact")
    elif mode == "simple":
        kw.update(impl=dev.IMPL_SIMPLE, arith="exact")
    else:
        kw.update(arith=mode)
    cfa, develop = frames[0].cfa, frames[0].develop
    outs = []
    for compressed in (True, False):
        with dev.Stack(H, W, **kw) as st:
            for fr, m in zip(frames, mosaics):
                if compressed:
                    st.push_packed(fr, develop=develop)
                else:
                    st.push_mosaic(m, cfa, develop=develop)
            if compressed:
                assert st.ljpeg_status() == 0
            outs.append(st.finish())
    assert_same(mode, outs[0], outs[1])
    assert outs[0].any()


def test_mixed_pushes_and_the_status_word(dev, stack_files, bad_file):
    """compressed, packed, mosaic and BGR pushes on one handle; a zero-copy compressed push out of pinned memory; the status
    word is zero, turns non-zero behind a short-stream frame and is cleared by the read"""
    from shinestacker_amd import debayer
    _, _, plain, frames, mosaics = stack_files
    cfa, develop = frames[0].cfa, frames[0].develop
    packed = dng.read(plain[1])
    pinned = dev.host_alloc(frames[2].span.shape, np.uint8)
    pinned[:] = frames[2].span
    zero = dng.DngFrame(frames[2].path, frames[2].layout, pinned, frames[2].cfa, frames[2].develop, None, 1, ())
    bgr3 = debayer(mosaics[3], cfa, develop=develop)
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=16, arith="separable") as st:
        assert st.ljpeg_status() == 0                   # (a handle that never took a compressed frame)
        st.push_packed(frames[0], develop=develop)
        st.push_packed(packed, develop=develop)
        st.push_packed(zero, zero_copy=True, develop=develop)
        st.push_frame(bgr3)
        st.push_mosaic(mosaics[0], cfa, develop=develop)
        st.push_packed(frames[1], develop=develop)
        st.wait_uploads()
        assert st.ljpeg_status() == 0
        got = st.finish()
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=16, arith="separable") as st:
        for m in (mosaics[0], mosaics[1], mosaics[2], mosaics[3], mosaics[0], mosaics[1]):
            st.push_mosaic(m, cfa, develop=develop)
        want = st.finish()
    assert_same("mixed", got, want)
    bad = dng.read(bad_file)
    for kw in (dict(arith="separable"), dict(float_type=dev.MI_F64, arith="exact")):
        with dev.Stack(H, W, in_dtype=np.uint16, min_size=16, **kw) as st:
            st.push_packed(frames[0], develop=develop)
            assert st.ljpeg_status() == 0
            st.push_packed(bad, develop=develop)
            st.push_packed(frames[1], develop=develop)
            assert st.ljpeg_status() == R.OVERRUN and st.ljpeg_status() == 0
    with dev.Stack(H + 2, W, in_dtype=np.uint16) as st:
        with pytest.raises(ValueError, match="mosaic shape"):
            st.push_packed(frames[0])


def test_develop_and_frames_device(dev, stack_files):
    _, comp, plain, frames, mosaics = stack_files
    for p, q in zip(comp, plain):
        assert_same(("develop", p), dng.develop(dng.read(p)), dng.develop(dng.read(q)))
    assert_same("plain", dng.develop(frames[0], develop=None, lens=None), dng.develop(dng.read(plain[0]), develop=None, lens=None))
    fb = H * W * 3 * 2
    a, b = dev.DeviceBuffer(N * fb), dev.DeviceBuffer(N * fb)
    try:
        assert dng.frames_device(comp, a.ptr) == dng.frames_device(plain, b.ptr) == (H, W, np.dtype(np.uint16))
        assert_same("frames_device", a.download((N, H, W, 3), np.uint16), b.download((N, H, W, 3), np.uint16))
    finally:
        a.free()
        b.free()


class _Quiet:
    """the little of an action a stacker talks to"""
    id, name = 0, "quiet"

    def sub_message_r(self, *a, **k):
        pass

    def callback(self, *a, **k):
        return None


@pytest.mark.parametrize("lens", [None, "own"], ids=["no-lens", "lens"])
def test_pyramid_stack_reads_compressed_dng_paths(dev, stack_files, bad_file, lens):
    from shinestacker_amd import Lens, PyramidStack
    _, comp, plain, _, _ = stack_files
    L = None if lens is None else Lens.distortion(-0.08, 0.01)
    outs = []
    for paths in (comp, plain):
        algo = PyramidStack(min_size=16, raw=dng.Raw(lens=L))
        try:
            algo.process = _Quiet()
            outs.append(algo.focus_stack(paths))
        finally:
            algo.close()
    assert_same(("focus_stack", lens), outs[0], outs[1])
    # a stack with a frame that does not decode is an error, not a picture
    algo = PyramidStack(min_size=16, raw=dng.Raw(lens=L))
    try:
        algo.process = _Quiet()
        with pytest.raises(ImageLoadError, match="lossless JPEG"):
            algo.focus_stack([comp[0], bad_file])
    finally:
        algo.close()


def test_focus_stack_and_combined_actions_on_folders_of_compressed_dngs(dev, stack_files, tmp_path):
    import shutil
    from shinestacker_amd import AlignFrames, CombinedActions, FocusStack, PyramidStack, StackJob
    from shinestacker_amd.align import ecc_estimator
    from shinestacker_amd.imageio import read_img
    _, comp, plain, _, _ = stack_files
    work = str(tmp_path)
    for name, paths in (("ljpeg", comp), ("plain", plain)):
        os.makedirs(os.path.join(work, name))
        for p in paths:
            shutil.copy(p, os.path.join(work, name))
    job = StackJob("job", work, input_path="ljpeg")
    for name in ("ljpeg", "plain"):
        job.add_action(FocusStack("stack-" + name, PyramidStack(min_size=16), input_path=name, output_path="out-" + name, raw=dng.Raw()))
        job.add_action(CombinedActions("align-" + name, [AlignFrames(estimator=ecc_estimator(), subsample=1)], input_path=name,
                                       output_path="aligned-" + name, raw=dng.Raw()))
    job.run()
    for kind, count in (("out", 1), ("aligned", N)):
        names = sorted(os.listdir(os.path.join(work, kind + "-plain")))
        assert len(names) == count and sorted(os.listdir(os.path.join(work, kind + "-ljpeg"))) == names
        for n in names:
            assert_same((kind, n), read_img(os.path.join(work, kind + "-ljpeg", n)), read_img(os.path.join(work, kind + "-plain", n)))
