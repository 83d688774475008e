"""GPU: mosaic_radial_gain and frame_finish (csrc/kernels_finish.hpp) equal their NumPy restatement (tests/finish_restatement.py)
bit for bit on the cases of tests/finish_cases.py -- which test_finish_host.py shows to be meaningful -- in host form and in device
form; and the layers above (dng.unpack, dng.develop, dng.frames_device, PyramidStack(raw=) and FocusStack on a folder of .dng
files at orientation 6 with a crop and a vignette) equal the same work done by hand.  Every comparison is array_equal."""
import os

import numpy as np
import pytest

import dng_cases as DC
import finish_cases as FC
import finish_restatement as R
import unpack_restatement as UR
from shinestacker_amd import Cfa, dng
from shinestacker_amd import demosaic as dm

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of the device buffer a kernel writes


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


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.shape, want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def _wait(dev, side, stream):
    if stream:
        side.sync()
    else:
        dev.check(dev.load().mi_device_synchronize(0))


# ---------------------------------------------------------------------------------------------- mosaic_radial_gain
@pytest.mark.parametrize("case", FC.RADIAL_CASES, ids=repr)
def test_radial_gain_equals_the_restatement(dev, side, case):
    """the host form; the device form between guard bands on the null stream, on a handle's stream, and with the mosaic
    starting off the 16-byte grid (other windows, the same sites)"""
    cfa = Cfa("RGGB", black=case.black)
    gain = dng.RadialGain(case.k, case.centre)
    m = case.mosaic()
    want = R.radial_gain(m, case.black, *gain.centre2(), gain.table())
    assert not np.array_equal(want, m)
    assert_same((case, "host"), dm.radial_gain(m, cfa, gain), want)
    item = case.dtype.itemsize
    buf = dev.DeviceBuffer(m.nbytes + 2 * GUARD + 16)
    try:
        for stream, shift in ((None, 0), (side.stream, 0), (None, 3 * item)):
            raw = np.full(buf.nbytes, 0xA5, np.uint8)
            at = GUARD + shift
            raw[at:at + m.nbytes] = m.reshape(-1).view(np.uint8)
            buf.upload(raw)
            dm.radial_gain_device(buf.ptr + at, case.h, case.w, case.dtype, cfa, gain, stream=stream)
            _wait(dev, side, stream)
            back = buf.download((buf.nbytes,), np.uint8)
            assert (back[:at] == 0xA5).all() and (back[at + m.nbytes:] == 0xA5).all(), "the guard band around the mosaic was written"
            assert_same((case, "device", stream, shift), back[at:at + m.nbytes].copy().view(case.dtype).reshape(m.shape), want)
    finally:
        buf.free()
        gain.close()


# ---------------------------------------------------------------------------------------------- frame_finish
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("case", FC.FINISH_CASES, ids=repr)
def test_frame_finish_equals_the_restatement(dev, side, case, dtype):
    """all eight orientations: the host form; the device form into guard bands on the null stream, on a handle's stream, and
    with source and destination off the 16-byte grid"""
    a = case.frame(dtype)
    item = a.itemsize
    src = dev.DeviceBuffer(a.nbytes + 32)
    dst = dev.DeviceBuffer(a.nbytes + 2 * GUARD + 16)
    try:
        for shift in (0, 5 * item):
            src.upload(np.concatenate([np.zeros(shift, np.uint8), a.reshape(-1).view(np.uint8)]))
            for o in FC.ORIENTATIONS:
                fin = dng.Finish(crop=case.crop, orientation=o)
                want = R.finish(a, case.crop, o)
                assert want.shape[:2] == fin.finished_shape(a.shape[:2])
                if shift == 0:
                    assert_same((case, o, "host"), dm.finish_frame(a, fin), want)
                for stream in ((None, side.stream) if shift == 0 else (None,)):
                    at = GUARD + shift
                    dst.upload(np.full(dst.nbytes, 0xA5, np.uint8))
                    dm.finish_frame_device(src.ptr + shift, dst.ptr + at, case.h, case.w, dtype, fin, stream=stream)
                    _wait(dev, side, stream)
                    back = dst.download((dst.nbytes,), np.uint8)
                    assert (back[:at] == 0xA5).all() and (back[at + want.nbytes:] == 0xA5).all(), "the guard band around the frame was written"
                    assert_same((case, o, "device", stream, shift), back[at:at + want.nbytes].copy().view(a.dtype).reshape(want.shape), want)
    finally:
        src.free()
        dst.free()


# ---------------------------------------------------------------------------------------------- the layers above
H, W, N = 72, 104, 3
CROP = (4, 6, 60, 90)                       # (y, x, h, w): DefaultCropOrigin (6, 4), DefaultCropSize (90, 60)
ORIENTATION = 6


@pytest.fixture(scope="module")
def stack_files(oracle, tmp_path_factory):
    """three 12-bit DNGs of one synthetic focus stack at orientation 6, with a default crop and, in OpcodeList3, a
    WarpRectilinear followed by a FixVignetteRadial; their frames and restated mosaics"""
    d = tmp_path_factory.mktemp("finish")
    paths, frames, mosaics = [], [], []
    for f in range(N):
        bgr = oracle.synth_frame_numpy(H, W, f, N).astype(np.int64)
        stored = dm.mosaic_of(256 + bgr * 10, "GRBG")                 # 12-bit samples over a black level of 256, room for the gain
        p = str(d / f"f{f:02d}.dng")
        DC.write_dng(p, stored, 12, rows_per_strip=7, pattern="GRBG", black=(256,), neutral=(0.55, 1.0, 0.7),
                     matrices={1: (DC.XYZ_D65_MATRIX, 21)}, opcodes3=[DC.WARP, FC.fix_vignette_radial(FC.VIG, (0.5, 0.5))],
                     orientation=ORIENTATION, extra=FC.default_crop((CROP[1], CROP[0]), (CROP[3], CROP[2])))
        paths.append(p)
        frames.append(dng.read(p))
        mosaics.append(UR.unpack_layout(frames[-1].span, frames[-1].layout))
    f0 = frames[0]
    assert f0.finish.crop == CROP and f0.finish.orientation == ORIENTATION and f0.finish.vignette.after_warp and f0.lens is not None
    assert f0.finish.skipped == () and f0.finished_shape() == (CROP[3], CROP[2])
    return str(d), paths, frames, mosaics


def _by_hand(frame, mosaic, lens="own", develop="own"):
    """correct the mosaic with the restatement, develop it as ever, crop and turn with NumPy"""
    fin = frame.finish
    ln = frame.lens if lens == "own" else lens
    m = R.radial_gain(mosaic, frame.cfa.black, *fin.vignette.centre2(), fin.vignette.table(ln))
    return R.finish(dm.debayer(m, frame.cfa, develop=frame.develop if develop == "own" else develop, lens=ln), fin.crop, fin.orientation)


def test_unpack_develop_and_frames_device_with_a_finish(dev, stack_files):
    _, paths, frames, mosaics = stack_files
    f, m = frames[0], mosaics[0]
    gain = f.finish.vignette
    # unpack: the vignette alone, and no lens behind it here: the polynomial's own table
    assert_same("unpack", dng.unpack(f, finish="auto"), R.radial_gain(m, f.cfa.black, *gain.centre2(), gain.table()))
    assert_same("unpack, off", dng.unpack(f), m)
    want = _by_hand(f, m)
    assert want.shape == (CROP[3], CROP[2], 3)
    assert_same("develop auto", dng.develop(f, finish="auto"), want)
    assert_same("develop, own object", dng.develop(f, finish=dng.Finish(gain, CROP, ORIENTATION)), want)
    assert_same("develop, no lens", dng.develop(f, lens=None, finish="auto"), _by_hand(f, m, lens=None))
    assert_same("develop, plain demosaic", dng.develop(f, develop=None, finish="auto"), _by_hand(f, m, develop=None))
    assert_same("develop, geometry only", dng.develop(f, finish=dng.Finish(crop=CROP, orientation=3)),
                R.finish(dm.debayer(m, f.cfa, develop=f.develop, lens=f.lens), CROP, 3))
    assert_same("develop, vignette only", dng.develop(f, finish=dng.Finish(gain)),
                dm.debayer(R.radial_gain(m, f.cfa.black, *gain.centre2(), gain.table(f.lens)), f.cfa, develop=f.develop, lens=f.lens))
    # finish=None: what it was
    assert_same("develop, off", dng.develop(f), dm.debayer(m, f.cfa, develop=f.develop, lens=f.lens))
    fb = want.nbytes
    out = dev.DeviceBuffer(N * H * W * 3 * 2)
    try:
        assert dng.frames_device(paths, out.ptr, finish="auto") == (CROP[3], CROP[2], np.dtype(np.uint16))
        for i in range(N):
            assert_same(("frames_device", i), out.download(want.shape, np.uint16, i * fb), _by_hand(frames[i], mosaics[i]))
        assert dng.frames_device(paths, out.ptr) == (H, W, np.dtype(np.uint16))
        assert_same("frames_device, off", out.download((H, W, 3), np.uint16, H * W * 6), dng.develop(frames[1]))
    finally:
        out.free()


class _Quiet:
    """the little of an action a stacker talks to"""
    id, name = 0, "quiet"

    def sub_message_r(self, *a, **k):
        pass

    def callback(self, *a, **k):
        return None


def test_a_stack_of_dngs_comes_out_finished(dev, stack_files, tmp_path):
    """PyramidStack(raw=Raw(finish="auto")) and FocusStack on the folder equal the stack of the frames finished by hand; with
    finish=None the same folder gives what it gave before: the stack of the stored frames"""
    import shutil
    from shinestacker_amd import FocusStack, PyramidStack, StackJob
    from shinestacker_amd.imageio import read_img
    _, paths, frames, mosaics = stack_files
    plain = PyramidStack(min_size=16)
    algo = PyramidStack(min_size=16, raw=dng.Raw(finish="auto"))
    off = PyramidStack(min_size=16, raw=dng.Raw())
    try:
        want = plain.focus_stack_arrays([_by_hand(f, m) for f, m in zip(frames, mosaics)])
        before = plain.focus_stack_arrays([dm.debayer(m, f.cfa, develop=f.develop, lens=f.lens) for f, m in zip(frames, mosaics)])
        assert want.shape == (CROP[3], CROP[2], 3) and before.shape == (H, W, 3)
        algo.process = off.process = _Quiet()
        assert_same("focus_stack", algo.focus_stack(paths), want)
        assert_same("focus_stack, off", off.focus_stack(paths), before)
    finally:
        for a in (plain, algo, off):
            a.close()
    work = str(tmp_path)
    os.makedirs(os.path.join(work, "in"))
    for p in paths:
        shutil.copy(p, os.path.join(work, "in"))
    job = StackJob("job", work, input_path="in")
    job.add_action(FocusStack("stack", PyramidStack(min_size=16), input_path="in", output_path="out", raw=dng.Raw(finish="auto"),
                              depth_composite_path="composite"))
    job.add_action(FocusStack("stack-off", PyramidStack(min_size=16), input_path="in", output_path="out-off", raw=dng.Raw()))
    job.run()
    names = sorted(os.listdir(os.path.join(work, "out")))
    assert len(names) == 1 and names[0].endswith("f00.tif"), names
    assert_same("FocusStack", read_img(os.path.join(work, "out", names[0])), want)
    assert read_img(os.path.join(work, "composite", names[0])).shape == want.shape      # derived outputs: the finished geometry
    assert_same("FocusStack, off", read_img(os.path.join(work, "out-off", names[0])), before)
