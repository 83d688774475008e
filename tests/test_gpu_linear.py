"""GPU: linear_develop (csrc/kernels_linear.hpp) equals its NumPy restatement (tests/linear_restatement.py) bit for bit on the
shapes of tests/linear_cases.py -- which test_linear_host.py shows to hit the paths they name -- in host form and in device
form between guard bands, from aligned and from misaligned base pointers; dng.unpack of the written LinearRaw files equals what
the writer stored; and the layers above (dng.develop, dng.frames_device, PyramidStack(raw=), FocusStack on a folder of linear
.dng files, linear and CFA files in one folder) equal the same work done by hand.  Every comparison is array_equal."""
import os

import numpy as np
import pytest

import dng_cases as DC
import linear_cases as LC
import linear_restatement as LR
from shinestacker_amd import demosaic, dng

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of the device buffer the kernel writes


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def _levels(dtype, spp):
    """a Linear with levels that differ per channel, a white below the dtype's maximum, gains that reach the clamp"""
    if np.dtype(dtype) == np.uint8:
        return demosaic.Linear(black=(16, 12, 20)[:spp], gains=(1.9, 1.0, 1.45)[:spp], white=250, spp=spp)
    return demosaic.Linear(black=(4096, 4000, 4200)[:spp], gains=(1.9, 1.0, 1.45)[:spp], white=64000, spp=spp)


def _develops(dtype):
    tone = demosaic.srgb_tone(dtype)
    return {"plain": None, "matrix": demosaic.Develop(matrix=LC.MATRIX), "matrix+tone": demosaic.Develop(matrix=LC.MATRIX, tone=tone)}


def _want(samples, lin, develop):
    black, gain_q, white, _ = lin.quantised(samples.dtype)
    mq = None if develop is None else develop.matrix_q
    tone = None if develop is None else develop.tone_table(samples.dtype)
    return LR.linear_develop(samples, black, gain_q, white, mq, tone)


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_linear_develop_equals_the_restatement(dev, dtype, spp):
    """every shape of the table, plain, with the matrix and with matrix and tone: the host form"""
    span = dev.linear_span(dtype)
    lin = _levels(dtype, spp)
    develops = _develops(dtype)
    try:
        for name, (h, w) in LC.kernel_shapes(dtype, span).items():
            a = LC.samples_for(h, w, spp, dtype, lin.black, lin.quantised(dtype)[2])
            for kind, d in develops.items():
                assert_same((name, kind), demosaic.develop_linear(a, lin, develop=d), _want(a, lin, d))
    finally:
        for d in develops.values():
            if d is not None:
                d.close()


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_device_form_between_guard_bands_and_off_alignment(dev, dtype, spp):
    """the device form writes h x w x 3 samples and not a byte more, from 4-byte aligned pointers (groups taken whole) and from
    pointers off that boundary (every group sample by sample): the same values"""
    item = np.dtype(dtype).itemsize
    span = dev.linear_span(dtype)
    lin = _levels(dtype, spp)
    d = _develops(dtype)["matrix+tone"]
    shapes = LC.kernel_shapes(dtype, span)
    try:
        for name in ("1x1", "3x5", "3x7", "span-1", "span+1"):
            h, w = shapes[name]
            a = LC.samples_for(h, w, spp, dtype, lin.black, lin.quantised(dtype)[2], seed=1)
            want = _want(a, lin, d)
            src = dev.DeviceBuffer(a.nbytes + 8)
            out = dev.DeviceBuffer(want.nbytes + 2 * GUARD + 8)
            try:
                for so, do in ((0, 0), (item, 0), (0, item), (item, item)):
                    src.upload(a, so)
                    out.upload(np.full(out.nbytes, 0xA5, np.uint8))
                    demosaic.develop_linear_device(src.ptr + so, out.ptr + GUARD + do, h, w, dtype, lin, develop=d)
                    dev.check(dev.load().mi_device_synchronize(0))
                    raw = out.download((out.nbytes,), np.uint8)
                    lo, hi = GUARD + do, GUARD + do + want.nbytes
                    assert (raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all(), (name, so, do, "the guard band was written")
                    assert_same((name, so, do), raw[lo:hi].copy().view(want.dtype).reshape(want.shape), want)
            finally:
                src.free()
                out.free()
    finally:
        d.close()


def test_lens_and_finish_run_behind_it(dev):
    from shinestacker_amd import Lens
    from shinestacker_amd.lens import correct
    lin = _levels(np.uint16, 3)
    a = LC.samples_for(24, 40, 3, np.uint16, lin.black, 64000, seed=2)
    d = _develops(np.uint16)["matrix+tone"]
    L = Lens.distortion(-0.08, 0.01)
    fin = dng.Finish(crop=(2, 3, 20, 30), orientation=6)
    try:
        base = demosaic.develop_linear(a, lin, develop=d)
        assert_same("base", base, _want(a, lin, d))
        assert_same("lens", demosaic.develop_linear(a, lin, develop=d, lens=L), correct(base, L))
        assert_same("finish", demosaic.develop_linear(a, lin, develop=d, finish=fin), demosaic.finish_frame(base, fin))
        assert_same("both", demosaic.develop_linear(a, lin, develop=d, lens=L, finish=fin), demosaic.finish_frame(correct(base, L), fin))
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- files
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("linear")
    out = {}
    for c in LC.FILE_CASES:
        c.write(str(d / (c.name + ".dng")))
        out[c.name] = dng.read(str(d / (c.name + ".dng")))
    return out


@pytest.mark.parametrize("case", LC.FILE_CASES, ids=repr)
def test_unpack_returns_what_the_writer_stored(dev, files, case):
    """H x W x 3 RGB samples (H x W at one sample per pixel): raw_unpack on the layout in samples, unchanged"""
    frame = files[case.name]
    got = dng.unpack(frame)
    assert_same(case, got, case.expected())
    black, gain_q = case.linear_ints()
    want = LR.linear_develop(got, black, gain_q)
    assert_same((case, "plain"), dng.develop(frame, develop=None, lens=None), want)
    if frame.develop is not None:
        want = LR.linear_develop(got, black, gain_q, None, frame.develop.matrix_q, frame.develop.tone_table(case.dtype))
        assert_same((case, "auto"), dng.develop(frame), want)
        frame.develop.close()


# ---------------------------------------------------------------------------------------------- stacks
H, W, N = 24, 40, 4


@pytest.fixture(scope="module")
def stack_files(oracle, tmp_path_factory):
    """four 12-bit LinearRaw DNGs of one synthetic focus stack (colour matrix, white balance, black level, a default crop and an
    orientation), their frames and their samples"""
    d = tmp_path_factory.mktemp("stack")
    paths, frames, samples = [], [], []
    for f in range(N):
        bgr = oracle.synth_frame_numpy(H, W, f, N).astype(np.int64)
        stored = 256 + bgr[:, :, ::-1] * 15                             # 12-bit RGB samples over a black level of 256
        p = str(d / f"f{f:02d}.dng")
        LC.write_linear(p, stored, 12, rows_per_strip=7, odd_start=True, black=(256,), neutral=(0.55, 1.0, 0.7),
                        matrices={1: (DC.XYZ_D65_MATRIX, 21)}, orientation=6, extra={50719: (4, [2, 1]), 50720: (4, [36, 20])})
        paths.append(p)
        frames.append(dng.read(p))
        samples.append((stored << 4).astype(np.uint16))
    return str(d), paths, frames, samples


def _by_hand(frames, samples, finish=None):
    out = [demosaic.develop_linear(s, f.linear, develop=f.develop) for f, s in zip(frames, samples)]
    return out if finish is None else [demosaic.finish_frame(o, f.finish) for f, o in zip(frames, out)]


def test_develop_and_frames_device(dev, stack_files):
    _, paths, frames, samples = stack_files
    hand = _by_hand(frames, samples)
    assert_same("unpack", dng.unpack(frames[0]), samples[0])
    assert_same("develop", dng.develop(frames[0]), hand[0])
    assert_same("develop, by the restatement", hand[0], LR.linear_develop(samples[0], frames[0].linear.black, frames[0].linear.gain_q, None,
                                                                         frames[0].develop.matrix_q, frames[0].develop.tone_table(np.uint16)))
    finished = _by_hand(frames, samples, "auto")
    assert finished[0].shape == (36, 20, 3) and frames[0].finish.crop == (1, 2, 20, 36)
    assert_same("finish", dng.develop(frames[0], finish="auto"), finished[0])
    assert_same("corrections auto: nothing to apply", dng.develop(frames[0], corrections="auto"), hand[0])
    for fin, want, shape in ((None, hand, (H, W)), ("auto", finished, (36, 20))):
        fb = shape[0] * shape[1] * 3 * 2
        out = dev.DeviceBuffer(N * fb)
        try:
            assert dng.frames_device(paths, out.ptr, finish=fin) == shape + (np.dtype(np.uint16),)
            for i in range(N):
                assert_same(("frames_device", fin, i), out.download(shape + (3,), np.uint16, i * fb), want[i])
        finally:
            out.free()


class _Quiet:
    id, name = 0, "quiet"

    def sub_message_r(self, *a, **k):
        pass

    def callback(self, *a, **k):
        return None


@pytest.mark.parametrize("finish", [None, "auto"], ids=["stored", "finished"])
def test_pyramid_stack_reads_linear_paths(dev, stack_files, finish):
    from shinestacker_amd import PyramidStack
    _, paths, frames, samples = stack_files
    algo = PyramidStack(min_size=8, raw=dng.Raw(finish=finish))
    plain = PyramidStack(min_size=8)
    try:
        algo.process = _Quiet()
        assert_same(("focus_stack", finish), algo.focus_stack(paths), plain.focus_stack_arrays(_by_hand(frames, samples, finish)))
    finally:
        algo.close()
        plain.close()


@pytest.mark.parametrize("finish", [None, "auto"], ids=["stored", "finished"])
def test_focus_stack_on_a_folder_of_linear_dngs(dev, stack_files, tmp_path, finish):
    """FocusStack(raw=Raw()) on a folder of four 24 x 40 linear files writes a .tif equal to the same work by hand"""
    import shutil
    from shinestacker_amd import FocusStack, PyramidStack, StackJob
    from shinestacker_amd.imageio import read_img
    _, paths, frames, samples = stack_files
    work = str(tmp_path)
    os.makedirs(os.path.join(work, "in"))
    for p in paths:
        shutil.copy(p, os.path.join(work, "in"))
    job = StackJob("job", work, input_path="in")
    job.add_action(FocusStack("stack", PyramidStack(min_size=8), input_path="in", output_path="out", raw=dng.Raw(finish=finish)))
    job.run()
    names = sorted(os.listdir(os.path.join(work, "out")))
    assert len(names) == 1 and names[0].endswith("f00.tif"), names
    plain = PyramidStack(min_size=8)
    try:
        want = plain.focus_stack_arrays(_by_hand(frames, samples, finish))
    finally:
        plain.close()
    assert_same(("FocusStack", finish), read_img(os.path.join(work, "out", names[0])), want)


def test_linear_and_cfa_files_mix_in_one_folder(dev, stack_files, tmp_path):
    """shape and dtype agree: a CFA file between linear ones is demosaiced, the linear ones are not"""
    from shinestacker_amd import PyramidStack, debayer
    from shinestacker_amd.demosaic import mosaic_of
    import unpack_restatement as UR
    _, paths, frames, samples = stack_files
    stored = mosaic_of((samples[1] >> 4)[:, :, ::-1].astype(np.int64), "GRBG")
    p = str(tmp_path / "cfa.dng")
    DC.write_dng(p, stored, 12, pattern="GRBG", black=(256,), neutral=(0.55, 1.0, 0.7), matrices={1: (DC.XYZ_D65_MATRIX, 21)})
    cfa_frame = dng.read(p)
    mixed = [paths[0], p, paths[2]]
    hand = _by_hand(frames, samples)
    mid = debayer(UR.unpack_layout(cfa_frame.span, cfa_frame.layout), cfa_frame.cfa, develop=cfa_frame.develop)
    algo = PyramidStack(min_size=8, raw=dng.Raw())
    plain = PyramidStack(min_size=8)
    try:
        algo.process = _Quiet()
        assert_same("mixed", algo.focus_stack(mixed), plain.focus_stack_arrays([hand[0], mid, hand[2]]))
    finally:
        algo.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- three-component lossless JPEG
import ljpeg_restatement as JR  # noqa: E402


@pytest.fixture(scope="module")
def ljpeg3_files(tmp_path_factory):
    """{case name: (DngFrame, the restated H x 3W samples, the restated status)}: written, parsed and restated once"""
    d = tmp_path_factory.mktemp("ljpeg3")
    out = {}
    for c in LC.LJPEG3_CASES + [LC.LJPEG3_SHORT[0]]:
        c.write(str(d / (c.name + ".dng")))
        frame = dng.read(str(d / (c.name + ".dng")))
        want, status = JR.unpack_layout(frame.span, frame.layout)
        want.setflags(write=False)
        out[c.name] = (frame, want, status)
    return out


@pytest.mark.parametrize("case", LC.LJPEG3_CASES, ids=repr)
def test_raw_ljpeg3_equals_the_restatement(dev, ljpeg3_files, case):
    """the host form through dng.unpack, and the device form between guard bands with its status words"""
    frame, want, status = ljpeg3_files[case.name]
    assert not status.any()
    h, w = frame.shape
    got = dng.unpack(frame)
    assert_same((case, "host"), got, want.reshape(h, w, 3))
    assert_same((case, "what the writer stored"), got, case.expected_px())
    up = dng._Staged(frame, 0)
    out = dev.DeviceBuffer(want.nbytes + 2 * GUARD)
    try:
        out.upload(np.full(out.nbytes, 0xA5, np.uint8))
        up.unpack_into(frame.layout, out.ptr + GUARD, 0)
        dev.check(dev.load().mi_device_synchronize(0))
        up.check_status()
        raw = out.download((out.nbytes,), np.uint8)
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + want.nbytes:] == 0xA5).all(), "the guard band around the samples was written"
        assert_same((case, "device"), raw[GUARD:GUARD + want.nbytes].copy().view(want.dtype).reshape(want.shape), want)
    finally:
        out.free()
        up.buf.free()


def test_a_stream_cut_short_is_flagged_and_the_rest_stays_exact(dev, ljpeg3_files):
    from shinestacker_amd.errors import ImageLoadError
    case, seg, flag = LC.LJPEG3_SHORT
    frame, want, status = ljpeg3_files[case.name]
    assert flag == dev.LJPEG_OVERRUN and status.tolist() == [flag if k == seg else 0 for k in range(len(status))]
    with pytest.raises(ImageLoadError, match=f"segment {seg} did not decode"):
        dng.unpack(frame)
    lay = frame.layout
    span = dng.host_span(frame)
    out = np.zeros((lay.height, lay.width), lay.dtype)
    got_status = np.zeros(len(lay.segments), np.uint32)
    L = lay.struct()
    dev.check(dev.load().mi_raw_ljpeg3(0, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, dev.C.byref(L), None, out.ctypes.data,
                                       got_status.ctypes.data))
    assert got_status.tolist() == status.tolist()
    rows = np.ones(lay.height, bool)
    rows[seg * lay.seg_height:(seg + 1) * lay.seg_height] = False
    assert_same("every other segment", out[rows], want[rows])


def test_compressed_linear_files_stack(dev, stack_files, tmp_path):
    """the same four frames written as lossless-JPEG tiles stack to the same picture as the packed files"""
    from shinestacker_amd import PyramidStack
    _, paths, frames, samples = stack_files
    cpaths = []
    for i, s in enumerate(samples):
        p = str(tmp_path / f"c{i:02d}.dng")
        LC.write_linear_ljpeg(p, (s >> 4).astype(np.int64), 12, tile=(16, 16), predictor=1 + i, black=(256,), neutral=(0.55, 1.0, 0.7),
                              matrices={1: (DC.XYZ_D65_MATRIX, 21)})
        cpaths.append(p)
        assert_same(("unpack", i), dng.unpack(dng.read(p)), s)
    algo = PyramidStack(min_size=8, raw=dng.Raw())
    plain = PyramidStack(min_size=8)
    try:
        algo.process = _Quiet()
        assert_same("compressed", algo.focus_stack(cpaths), plain.focus_stack_arrays(_by_hand(frames, samples)))
    finally:
        algo.close()
        plain.close()


def test_a_descriptor_the_host_refuses_is_flagged_on_the_device_and_nothing_is_written(dev, ljpeg3_files):
    """the device form cannot read descriptors that lie in device memory: the kernel flags what mi_raw_ljpeg3 would refuse
    (MI_LJPEG_UNDECODED), decodes nothing of that segment and leaves its samples as they were"""
    import copy
    frame, want, _ = ljpeg3_files["14bit-strips-of-3-short-last"]
    lay = copy.copy(frame.layout)
    lay.segments = frame.layout.segments.copy()
    lay.segments["ncomp"][1] = 2
    bad = dng.DngFrame(frame.path, lay, frame.span, None, None, None, 1, (), linear=frame.linear)
    up = dng._Staged(bad, 0)
    out = dev.DeviceBuffer(want.nbytes)
    try:
        out.upload(np.full(out.nbytes, 0xA5, np.uint8))
        up.unpack_into(lay, out.ptr, 0)
        dev.check(dev.load().mi_device_synchronize(0))
        assert up.buf.download((up.nseg,), np.uint32, up.status_at).tolist() == [0, dev.LJPEG_UNDECODED, 0]
        got = out.download(want.shape, want.dtype)
        assert (got[3:6].view(np.uint8) == 0xA5).all()
        assert_same("the other strips", np.delete(got, [3, 4, 5], axis=0), np.delete(want, [3, 4, 5], axis=0))
    finally:
        out.free()
        up.buf.free()
    span = dng.host_span(frame)
    L = lay.struct()
    rc = dev.load().mi_raw_ljpeg3(0, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, dev.C.byref(L), None, got.ctypes.data, None)
    assert rc == dev.MI_ERR_INVALID and b"segs[1].ncomp must be 3 (got 2)" in dev.load().mi_last_error()


# ---------------------------------------------------------------------------------------------- the ingest path: Stack.push_packed
@pytest.fixture(scope="module")
def compressed_files(stack_files, tmp_path_factory):
    """the four frames of stack_files once more as lossless-JPEG tiles of three components (16 x 16 pixels, predictors 1 to 4)"""
    _, _, frames, samples = stack_files
    d = tmp_path_factory.mktemp("cstack")
    out = []
    for i, s in enumerate(samples):
        p = str(d / f"c{i:02d}.dng")
        LC.write_linear_ljpeg(p, (s >> 4).astype(np.int64), 12, tile=(16, 16), predictor=1 + i, black=(256,), neutral=(0.55, 1.0, 0.7),
                              matrices={1: (DC.XYZ_D65_MATRIX, 21)})
        out.append(dng.read(p))
    return out


def _stack_kw(dev, mode):
    kw = dict(in_dtype=np.uint16, min_size=8)
    if mode == "float-64":
        kw.update(float_type=dev.MI_F64, arith="exact")
    elif mode == "simple":
        kw.update(impl=dev.IMPL_SIMPLE, arith="exact")
    else:
        kw.update(arith=mode)
    return kw


@pytest.mark.parametrize("mode", ["separable", "exact", "float-64", "simple"])
@pytest.mark.parametrize("form", ["packed", "compressed"])
@pytest.mark.parametrize("extras", ["plain", "developed"])
def test_push_packed_of_linear_frames_equals_pushes_of_the_frames_developed_by_hand(dev, stack_files, compressed_files, mode, form, extras):
    """the one ingest path (csrc/mosaic_host.hpp): the span up, raw_unpack or raw_ljpeg3 into a slot of H x W x 3 samples,
    linear_develop into the batch -- on the asynchronous route (more frames than slots would need more files: four frames fill
    the four slots once) and on the synchronous one of float-64 and simple handles"""
    _, _, frames, samples = stack_files
    src = frames if form == "packed" else compressed_files
    develop = frames[0].develop if extras == "developed" else None
    hand = [demosaic.develop_linear(s, f.linear, develop=develop) for f, s in zip(frames, samples)]
    outs = []
    for packed in (True, False):
        with dev.Stack(H, W, **_stack_kw(dev, mode)) as st:
            for fr, bgr in zip(src, hand):
                if packed:
                    st.push_packed(fr, develop=develop)
                else:
                    st.push_frame(bgr)
            if packed:
                assert st.ljpeg_status() == 0
            outs.append(st.finish())
    assert_same((mode, form, extras), outs[0], outs[1])
    assert outs[0].any()


def test_linear_cfa_and_bgr_pushes_mix_on_one_handle_and_the_slots_cycle(dev, stack_files, compressed_files, tmp_path):
    """nine pushes on one handle -- more than twice the stage's four slots, so every linear slot is reused behind its
    evSlotFree -- of packed linear, compressed linear, CFA (packed: a mosaic slot of one sample per pixel beside the linear
    ones of three) and BGR frames, a site correction held by the handle (it touches the CFA frame only), and a one-sample
    linear frame (a linear slot used at a third of its capacity)"""
    import unpack_restatement as UR
    from shinestacker_amd import debayer
    from shinestacker_amd.demosaic import mosaic_of
    _, _, frames, samples = stack_files
    develop = frames[0].develop
    hand = [demosaic.develop_linear(s, f.linear, develop=develop) for f, s in zip(frames, samples)]
    p = str(tmp_path / "cfa.dng")
    DC.write_dng(p, mosaic_of((samples[1] >> 4)[:, :, ::-1].astype(np.int64), "GRBG"), 12, pattern="GRBG", black=(256,), neutral=(0.55, 1.0, 0.7),
                 matrices={1: (DC.XYZ_D65_MATRIX, 21)})
    cfa = dng.read(p)
    sc = dng.SiteCorrections(black_h=np.arange(W) % 3, black_v=np.arange(H) % 2)
    mosaic = UR.unpack_layout(cfa.span, cfa.layout)
    cfa_hand = debayer(mosaic, cfa.cfa, develop=develop, corrections=sc)
    g = str(tmp_path / "grey.dng")
    grey = (samples[2][:, :, 1] >> 4).astype(np.int64)
    LC.write_linear(g, grey, 12, spp=1, black=(256,), rows_per_strip=5)
    gf = dng.read(g)
    grey_hand = demosaic.develop_linear((grey << 4).astype(np.uint16), gf.linear, develop=develop)
    order = [("lin", 0), ("clin", 1), ("cfa", None), ("lin", 2), ("bgr", 3), ("grey", None), ("clin", 3), ("lin", 1), ("clin", 0)]
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=8, arith="separable") as st:
        st.set_site_correction(sc)
        for kind, i in order:
            if kind == "lin":
                st.push_packed(frames[i], develop=develop)
            elif kind == "clin":
                st.push_packed(compressed_files[i], develop=develop)
            elif kind == "cfa":
                st.push_packed(cfa, develop=develop)
            elif kind == "grey":
                st.push_packed(gf, develop=develop)
            else:
                st.push_frame(hand[i])
        assert st.ljpeg_status() == 0
        got = st.finish()
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=8, arith="separable") as st:
        for kind, i in order:
            st.push_frame(cfa_hand if kind == "cfa" else grey_hand if kind == "grey" else hand[i])
        want = st.finish()
    assert_same("mixed", got, want)
    sc.close()


def test_push_packed_refuses_what_a_linear_frame_does_not_take(dev, stack_files):
    from shinestacker_amd.errors import InvalidOptionError
    _, _, frames, _ = stack_files
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=8) as st:
        for kw in (dict(calibration=demosaic.Calibration(dark=np.zeros((H, W), np.uint16))), dict(corrections=dng.SiteCorrections(bad_sites=[3])),
                   dict(develop=demosaic.Develop(defects=np.array([[1, 1]])))):
            with pytest.raises(InvalidOptionError, match="LinearRaw"):
                st.push_packed(frames[0], **kw)
    with dev.Stack(H + 1, W, in_dtype=np.uint16, min_size=8) as st:
        with pytest.raises(ValueError, match="frame shape"):
            st.push_packed(frames[0])
    with dev.Stack(H, W, in_dtype=np.uint8, min_size=8) as st:
        with pytest.raises(ValueError, match="frame dtype"):
            st.push_packed(frames[0])
    # the C boundary's own checks, with a handle
    lay, lin = frames[0].layout, frames[0].linear.struct(np.uint16)
    span, L, lib = dng.host_span(frames[0]), frames[0].layout.struct(), dev.load()

    def push(st, span_p=span.ctypes.data, segs=lay.offsets.ctypes.data, compressed=0, linear=dev.C.byref(lin), develop=None):
        return lib.mi_stack_push_linear(st._h, span_p, span.nbytes, segs, compressed, dev.C.byref(L), None, linear, develop, 0)

    def expect(rc, msg):
        assert rc == dev.MI_ERR_INVALID and msg in lib.mi_last_error(), (rc, msg, lib.mi_last_error())
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=8) as st:
        expect(push(st, span_p=None), b"null span")
        expect(push(st, segs=None), b"null seg_offsets")
        expect(push(st, segs=None, compressed=1), b"null segs")
        expect(push(st, linear=None), b"null linear")
        bad = frames[0].linear.struct(np.uint16)
        bad.spp = 2
        expect(push(st, linear=dev.C.byref(bad)), b"linear spp must be 1 or 3 (got 2)")
        one = demosaic.Linear(spp=1).struct(np.uint16)
        expect(push(st, linear=dev.C.byref(one)), b"layout height, width / spp and dtype must be the handle's")
        expect(push(st, develop=dev.C.byref(dev.DevelopStruct(4, (dev.C.c_int32 * 9)(), None))), b"unknown develop flags 4")
        assert push(st) == dev.MI_OK and st.finish().shape == (H, W, 3)
    with dev.Stack(H, W + 1, in_dtype=np.uint16, min_size=8) as st:
        expect(push(st), b"layout height, width / spp and dtype must be the handle's")
