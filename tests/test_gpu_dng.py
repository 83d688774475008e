"""GPU: raw_unpack (csrc/kernels_unpack.hpp) equals its NumPy restatement (tests/unpack_restatement.py) bit for bit on the cases
of tests/dng_cases.py -- which test_dng_host.py shows to be meaningful -- in host form and in device form; a packed push equals
the push of the restated mosaic; and the layers above (dng.develop, dng.frames_device, PyramidStack(raw=), FocusStack and
CombinedActions on folders of .dng files) equal the same work done by hand.  Every comparison is array_equal."""
import os

import numpy as np
import pytest

import dng_cases as DC
import unpack_restatement as R
from shinestacker_amd import dng

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
    """{case name: (DngFrame, the restated mosaic)} of the whole table: written, parsed and restated once"""
    d = tmp_path_factory.mktemp("dng")
    out = {}
    for c in DC.CASES:
        c.write(str(d / (c.name + ".dng")))
        frame = dng.read(str(d / (c.name + ".dng")))
        want = R.unpack_layout(frame.span, frame.layout)
        want.setflags(write=False)
        out[c.name] = (frame, want)
    return out


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


@pytest.mark.parametrize("case", DC.CASES, ids=repr)
def test_unpack_equals_the_restatement(dev, side, table, case):
    """the host form, and the device form between guard bands on the null stream and on a handle's stream"""
    frame, want = table[case.name]
    assert_same((case, "host"), dng.unpack(frame), want)
    lay = frame.layout
    up = dng._Staged(frame, 0)
    out = dev.DeviceBuffer(want.nbytes + 2 * GUARD)
    try:
        for stream in (None, side.stream):
            out.upload(np.full(out.nbytes, 0xA5, np.uint8))
            up.unpack_into(lay, out.ptr + GUARD, 0, stream)
            if stream:
                side.sync()
            else:
                dev.check(dev.load().mi_device_synchronize(0))
            raw = out.download((out.nbytes,), np.uint8)
            assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + want.nbytes:] == 0xA5).all(), "the guard band around the mosaic was written"
            assert_same((case, "device", stream), raw[GUARD:GUARD + want.nbytes].copy().view(want.dtype).reshape(want.shape), want)
        if want.dtype == np.uint16:      # an output that starts off the 16-byte boundary: other windows, the same samples
            out.upload(np.full(out.nbytes, 0xA5, np.uint8))
            up.unpack_into(lay, out.ptr + GUARD + 6, 0)
            dev.check(dev.load().mi_device_synchronize(0))
            raw = out.download((out.nbytes,), np.uint8)
            assert (raw[:GUARD + 6] == 0xA5).all() and (raw[GUARD + 6 + want.nbytes:] == 0xA5).all()
            assert_same((case, "device, off 6"), raw[GUARD + 6:GUARD + 6 + want.nbytes].copy().view(want.dtype).reshape(want.shape), want)
    finally:
        out.free()
        up.buf.free()


def test_offsets_outside_the_span_read_nothing(dev, table):
    """the kernel reads no byte at or beyond span_bytes, such bytes count as 0: the span is DECLARED 200 bytes shorter than
    the buffer that holds it, so every address stays inside the allocation"""
    frame, want = table["12bit-5x130"]
    lay = frame.layout
    up = dng._Staged(frame, 0)
    out = dev.DeviceBuffer(want.nbytes)
    try:
        short = frame.span.nbytes - 200
        dng.unpack_device(lay, up.buf.ptr, short, up.buf.ptr + up.seg_at, None, out.ptr)
        dev.check(dev.load().mi_device_synchronize(0))
        got = out.download(want.shape, want.dtype)
        cut = np.array(frame.span).copy()
        cut[short:] = 0
        assert_same("short span", got, R.unpack_layout(cut, lay))
        assert not np.array_equal(got, want)
    finally:
        out.free()
        up.buf.free()


# ---------------------------------------------------------------------------------------------- stacks
H, W, N = 72, 104, 4


@pytest.fixture(scope="module")
def stack_files(oracle, tmp_path_factory):
    """four 12-bit DNGs of one synthetic focus stack (colour matrix, white balance, black level), their frames and mosaics"""
    from shinestacker_amd.demosaic import mosaic_of
    d = tmp_path_factory.mktemp("stack")
    paths, frames, mosaics = [], [], []
    for f in range(N):
        bgr = oracle.synth_frame_numpy(H, W, f, N).astype(np.int64)
        stored = mosaic_of(256 + bgr * 15, "GRBG")                    # 12-bit samples over a black level of 256
        p = str(d / f"f{f:02d}.dng")
        DC.write_dng(p, stored, 12, rows_per_strip=7, odd_start=True, pattern="GRBG", black=(256,), neutral=(0.55, 1.0, 0.7),
                     matrices={1: (DC.XYZ_D65_MATRIX, 21)})
        paths.append(p)
        frames.append(dng.read(p))
        mosaics.append(R.unpack_layout(frames[-1].span, frames[-1].layout))
    assert all(np.array_equal(m, (mosaic_of(256 + oracle.synth_frame_numpy(H, W, f, N).astype(np.int64) * 15, "GRBG") << 4))
               for f, m in enumerate(mosaics))
    return str(d), paths, frames, mosaics


def _calibration(cfa):
    from shinestacker_amd import Calibration
    rng = np.random.default_rng(5)
    dark = (cfa.black[0] + rng.integers(0, 64, size=(H, W))).astype(np.uint16)
    flat = (30000 + rng.integers(0, 8000, size=(H, W))).astype(np.uint16)
    return Calibration(dark=dark, flat=flat)


@pytest.mark.parametrize("mode", ["separable", "exact", "float-64", "simple"])
@pytest.mark.parametrize("extras", ["plain", "developed", "calibrated"])
def test_push_packed_equals_push_mosaic(dev, stack_files, mode, extras):
    _, _, frames, mosaics = stack_files
    kw = dict(in_dtype=np.uint16, min_size=16)
    if mode == "float-64":
        kw.update(float_type=dev.MI_F64, arith="exact")
    elif mode == "simple":
        kw.update(impl=dev.IMPL_SIMPLE, arith="exact")
    else:
        kw.update(arith=mode)
    cfa = frames[0].cfa
    develop = frames[0].develop if extras != "plain" else None
    cal = _calibration(cfa) if extras == "calibrated" else None
    outs = []
    try:
        for packed in (True, False):
            with dev.Stack(H, W, **kw) as st:
                for fr, m in zip(frames, mosaics):
                    if packed:
                        st.push_packed(fr, develop=develop, calibration=cal)
                    else:
                        st.push_mosaic(m, cfa, develop=develop, calibration=cal)
                outs.append(st.finish())
    finally:
        if cal is not None:
            cal.close()
    assert_same((mode, extras), outs[0], outs[1])
    assert outs[0].any()


def test_mixed_pushes_and_a_growing_span(dev, stack_files, tmp_path):
    """packed, mosaic and BGR pushes on one handle, frame by frame; a later, larger span (gaps between its strips) makes the
    packed slot grow; a zero-copy packed push out of pinned memory"""
    from shinestacker_amd import debayer
    _, _, frames, mosaics = stack_files
    cfa, develop = frames[0].cfa, frames[0].develop
    stored = (mosaics[3] >> 4).astype(np.int64)
    big = str(tmp_path / "big.dng")
    DC.write_dng(big, stored, 12, rows_per_strip=5, gap=301, pattern="GRBG", black=(256,), neutral=(0.55, 1.0, 0.7),
                 matrices={1: (DC.XYZ_D65_MATRIX, 21)})
    bigframe = dng.read(big)
    assert bigframe.span.nbytes > frames[0].span.nbytes + 3000
    pinned = dev.host_alloc(frames[2].span.shape, np.uint8)
    pinned[:] = frames[2].span
    zero = dng.DngFrame(frames[2].path, frames[2].layout, pinned, frames[2].cfa, frames[2].develop, None, 1, ())
    bgr1 = debayer(mosaics[1], cfa, develop=develop)
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=16, arith="separable") as st:
        st.push_packed(frames[0], develop=develop)
        st.push_frame(bgr1)
        st.push_packed(zero, zero_copy=True, develop=develop)
        st.push_packed(bigframe, develop=develop)
        st.push_mosaic(mosaics[0], cfa, develop=develop)
        st.wait_uploads()
        got = st.finish()
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=16, arith="separable") as st:
        for m in (mosaics[0], mosaics[1], mosaics[2], mosaics[3], mosaics[0]):
            st.push_mosaic(m, cfa, develop=develop)
        want = st.finish()
    assert_same("mixed", got, want)
    with dev.Stack(H + 2, W, in_dtype=np.uint16) as st:
        with pytest.raises(ValueError, match="mosaic shape"):
            st.push_packed(frames[0])
    with dev.Stack(H, W, in_dtype=np.uint8) as st:
        with pytest.raises(ValueError, match="mosaic dtype"):
            st.push_packed(frames[0])


def test_develop_and_frames_device(dev, stack_files, table):
    from shinestacker_amd import Lens, debayer
    _, paths, frames, mosaics = stack_files
    f = frames[0]
    assert_same("auto", dng.develop(f), debayer(mosaics[0], f.cfa, develop=f.develop))
    assert_same("plain", dng.develop(f, develop=None), debayer(mosaics[0], f.cfa))
    L = Lens.distortion(-0.08, 0.01)
    assert_same("lens", dng.develop(f, lens=L), debayer(mosaics[0], f.cfa, develop=f.develop, lens=L))
    cal = _calibration(f.cfa)
    try:
        assert_same("calibrated", dng.develop(f, calibration=cal), debayer(mosaics[0], f.cfa, develop=f.develop, calibration=cal))
    finally:
        cal.close()
    # a file with its own lens opcode: "auto" applies it, None does not
    own, m = table["12bit-sub-ifd-colour"]
    assert own.lens is not None
    assert_same("own lens", dng.develop(own), debayer(m, own.cfa, develop=own.develop, lens=own.lens))
    assert_same("own lens off", dng.develop(own, lens=None), debayer(m, own.cfa, develop=own.develop))
    fb = H * W * 3 * 2
    out = dev.DeviceBuffer(N * fb)
    try:
        assert dng.frames_device(paths, out.ptr) == (H, W, np.dtype(np.uint16))
        for i in range(N):
            assert_same(("frames_device", i), out.download((H, W, 3), np.uint16, i * fb), dng.develop(frames[i]))
    finally:
        out.free()


@pytest.mark.parametrize("lens", [None, "own"], ids=["no-lens", "lens"])
def test_pyramid_stack_reads_dng_paths(dev, stack_files, lens):
    from shinestacker_amd import ImageLoadError, Lens, PyramidStack, debayer
    _, paths, frames, mosaics = stack_files
    L = None if lens is None else Lens.distortion(-0.08, 0.01)
    algo = PyramidStack(min_size=16, raw=dng.Raw(lens=L))
    plain = PyramidStack(min_size=16)
    try:
        algo.process = _Quiet()
        got = algo.focus_stack(paths)
        if L is None:
            want = plain.focus_stack_arrays(mosaics, mosaic=frames[0].cfa, develop=frames[0].develop)
        else:
            want = plain.focus_stack_arrays([debayer(m, frames[0].cfa, develop=frames[0].develop, lens=L) for m in mosaics])
        assert_same(("focus_stack", lens), got, want)
        plain.process = _Quiet()
        with pytest.raises(ImageLoadError):          # without raw= a .dng path is an unknown extension
            plain.focus_stack(paths)
    finally:
        algo.close()
        plain.close()


class _Quiet:
    """the little of an action a stacker talks to"""
    id, name = 0, "quiet"

    def sub_message_r(self, *a, **k):
        pass

    def callback(self, *a, **k):
        return None


def test_focus_stack_on_a_folder_of_dngs(dev, stack_files, tmp_path):
    """FocusStack(raw=dng.Raw()) writes a .tif equal to focus_stack_arrays(mosaic=) on the same data; without raw= the .dng
    files of a folder are ignored, as ever"""
    import shutil
    from shinestacker_amd import FocusStack, PyramidStack, StackJob
    from shinestacker_amd.imageio import read_img, write_img
    _, paths, frames, mosaics = stack_files
    work = str(tmp_path)
    os.makedirs(os.path.join(work, "in"))
    for p in paths:
        shutil.copy(p, os.path.join(work, "in"))
    job = StackJob("job", work, input_path="in")
    job.add_action(FocusStack("stack", PyramidStack(min_size=16), input_path="in", output_path="out", raw=dng.Raw(),
                              depth_composite_path="composite"))
    job.run()
    names = sorted(os.listdir(os.path.join(work, "out")))
    assert len(names) == 1 and names[0].endswith("f00.tif"), names
    plain = PyramidStack(min_size=16)
    try:
        want = plain.focus_stack_arrays(mosaics, mosaic=frames[0].cfa, develop=frames[0].develop)
    finally:
        plain.close()
    assert_same("FocusStack", read_img(os.path.join(work, "out", names[0])), want)
    assert sorted(os.listdir(os.path.join(work, "composite"))) == names         # every derived output is a .tif too
    # raw=None: a folder that also holds .dng files is scanned as ever
    tifs = [dng.develop(f) for f in frames[:2]]
    for i, t in enumerate(tifs):
        write_img(os.path.join(work, "in", f"t{i}.tif"), t)
    job = StackJob("job2", work, input_path="in")
    job.add_action(FocusStack("stack2", PyramidStack(min_size=16), input_path="in", output_path="out2"))
    job.run()
    names = sorted(os.listdir(os.path.join(work, "out2")))
    assert len(names) == 1 and names[0].endswith("t0.tif"), names
    plain = PyramidStack(min_size=16)
    try:
        assert_same("raw=None", read_img(os.path.join(work, "out2", names[0])), plain.focus_stack_arrays(tifs))
    finally:
        plain.close()


def test_combined_actions_job_on_dngs(dev, stack_files, tmp_path):
    """CombinedActions([AlignFrames], raw=) on .dng files == the existing job on the frames developed by hand"""
    import shutil
    from shinestacker_amd import AlignFrames, CombinedActions, StackJob
    from shinestacker_amd.align import ecc_estimator
    from shinestacker_amd.imageio import read_img, write_img
    _, paths, frames, _ = stack_files
    work = str(tmp_path)
    os.makedirs(os.path.join(work, "dng"))
    os.makedirs(os.path.join(work, "hand"))
    for p, f in zip(paths, frames):
        shutil.copy(p, os.path.join(work, "dng"))
        write_img(os.path.join(work, "hand", os.path.basename(p)[:-4] + ".tif"), dng.develop(f))

    def align():
        return AlignFrames(estimator=ecc_estimator(), subsample=1)
    job = StackJob("job", work, input_path="dng")
    job.add_action(CombinedActions("raw", [align()], input_path="dng", output_path="out-raw", raw=dng.Raw()))
    job.add_action(CombinedActions("hand", [align()], input_path="hand", output_path="out-hand"))
    job.run()
    names = sorted(os.listdir(os.path.join(work, "out-hand")))
    assert names == [f"f{i:02d}.tif" for i in range(N)] and sorted(os.listdir(os.path.join(work, "out-raw"))) == names
    for n in names:
        assert_same(("job", n), read_img(os.path.join(work, "out-raw", n)), read_img(os.path.join(work, "out-hand", n)))
