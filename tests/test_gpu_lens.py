"""GPU: the lens remap (csrc/kernels_lens.hpp) equals its NumPy restatement (tests/lens_restatement.py) bit for bit on the cases
of tests/lens_cases.py -- which test_lens_host.py shows to be meaningful -- in host form and in device form, with and without
the mask, on the null stream and on a handle's stream; and the layers above it (LensCorrection, the raw path, the two
pipelines) equal the remap applied by hand.  Every comparison is array_equal."""
import numpy as np
import pytest

import lens_cases as LC

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of a device buffer the kernel writes


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
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


class Resident:
    """a source frame in HBM, and a destination frame and a mask between guard bands"""

    def __init__(self, dev, frame):
        self.dev, self.frame = dev, frame
        h, w = frame.shape[:2]
        self.src = dev.DeviceBuffer(frame.nbytes)
        self.dst = dev.DeviceBuffer(frame.nbytes + 2 * GUARD)
        self.mask = dev.DeviceBuffer(h * w + 2 * GUARD)
        self.src.upload(frame)

    def run(self, side, lens, with_mask, stream=None):
        from shinestacker_amd.lens import correct_device
        f = self.frame
        h, w = f.shape[:2]
        for b in (self.dst, self.mask):
            b.upload(np.full(b.nbytes, 0xA5, np.uint8))
        correct_device(self.src.ptr, self.dst.ptr + GUARD, h, w, f.dtype, lens, stream=stream,
                       dev_mask=self.mask.ptr + GUARD if with_mask else None)
        if stream:
            side.sync()
        else:
            self.dev.check(self.dev.load().mi_device_synchronize(0))
        raw = self.dst.download((self.dst.nbytes,), np.uint8)
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + f.nbytes:] == 0xA5).all(), "the guard band around the frame was written"
        m = self.mask.download((self.mask.nbytes,), np.uint8)
        assert (m[:GUARD] == 0xA5).all() and (m[GUARD + h * w:] == 0xA5).all(), "the guard band around the mask was written"
        if not with_mask:
            assert (m == 0xA5).all(), "a mask was written without being asked for"
        assert np.array_equal(self.src.download(f.shape, f.dtype), f), "the source was written"
        return raw[GUARD:GUARD + f.nbytes].copy().view(f.dtype).reshape(f.shape), m[GUARD:GUARD + h * w].reshape(h, w).copy()

    def free(self):
        for b in (self.src, self.dst, self.mask):
            b.free()


@pytest.mark.parametrize("shape", LC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_remap_equals_the_restatement(dev, side, dtype, shape):
    """the whole case table at one shape and dtype: host form and device form, each with and without the mask"""
    from shinestacker_amd.lens import correct
    res = {k: Resident(dev, LC.frame(k, shape, dtype)) for k in LC.FRAMES}
    try:
        for i, (name, kind, fk) in enumerate(LC.cases(shape, dtype)):
            want, want_mask = LC.reference(name, kind, fk, shape, dtype)
            L = LC.lens_of(name, kind, shape)
            f = LC.frame(fk, shape, dtype)
            tag = (shape, np.dtype(dtype).name, name, kind, fk)
            got, mask = correct(f, L, return_mask=True)
            assert_same(tag + ("host, mask",), got, want)
            assert_same(tag + ("host, the mask",), mask, want_mask)
            assert_same(tag + ("host",), correct(f, L), want)
            got, mask = res[fk].run(side, L, True)
            assert_same(tag + ("device, mask",), got, want)
            assert_same(tag + ("device, the mask",), mask, want_mask)
            got, _ = res[fk].run(side, L, False, side.stream if i & 1 else None)
            assert_same(tag + ("device",), got, want)
    finally:
        for r in res.values():
            r.free()


def test_non_default_stream(dev, side):
    shape = LC.SHAPES[-1]
    for dtype in LC.DTYPES:
        r = Resident(dev, LC.frame("random", shape, dtype))
        try:
            for name in ("barrel", "CA", "mixed"):
                want, want_mask = LC.reference(name, "off", "random", shape, dtype)
                got, mask = r.run(side, LC.lens_of(name, "off", shape), True, side.stream)
                assert_same((name, "stream"), got, want)
                assert_same((name, "stream, the mask"), mask, want_mask)
        finally:
            r.free()


def test_largest_case(dev, side):
    """256 x 1024: many workgroups in both directions"""
    import lens_restatement as R
    from shinestacker_amd import Lens
    from shinestacker_amd.lens import correct
    shape = (256, 1024)
    for dtype in LC.DTYPES:
        f = LC.frame("random", shape, dtype)
        for k, c in ((LC.LENSES["barrel"], None), (LC.LENSES["mixed"], (700.25, 33.5))):
            want, want_mask = R.remap(f, k, c, return_mask=True)
            got, mask = correct(f, Lens(k, c), return_mask=True)
            assert_same((shape, "host"), got, want)
            assert_same((shape, "host, the mask"), mask, want_mask)


def test_source_and_destination_must_differ(dev):
    from shinestacker_amd.lens import correct_device
    buf = dev.DeviceBuffer(4 * 6 * 3)
    try:
        with pytest.raises(ValueError, match="distinct"):
            correct_device(buf.ptr, buf.ptr, 4, 6, np.uint8, LC.lens_of("barrel", "default", (4, 6)))
    finally:
        buf.free()


@pytest.mark.parametrize("dtype", LC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_sub_action_host_equals_device(dev, dtype):
    """LensCorrection.run_frame == run_frame_device (in place on a resident frame), with and without autoscale"""
    from shinestacker_amd import LensCorrection
    from shinestacker_amd.lens import correct
    shape = (33, 47)
    f = LC.frame("random", shape, dtype)
    for name, auto in (("outward", False), ("outward", True), ("CA", False)):
        L = LC.lens_of(name, "off", shape)
        step = LensCorrection(L, autoscale=auto)
        step.begin(None)
        host = step.run_frame(0, 0, f)
        buf = dev.DeviceBuffer(2 * f.nbytes)
        try:
            for i in range(2):                  # twice: the scratch frame is reused
                buf.upload(f, i * f.nbytes)
                step.run_frame_device(i, buf.ptr + i * f.nbytes, shape[0], shape[1], dtype)
            dev.check(dev.load().mi_device_synchronize(0))
            for i in range(2):
                assert_same((name, auto, i), buf.download(f.shape, dtype, i * f.nbytes), host)
        finally:
            step.end()
            buf.free()
        used = L.scaled(L.autoscale(*shape)) if auto else L
        assert_same((name, auto, "the lens used"), host, correct(f, used))
        assert not np.array_equal(host, f)
        if auto:
            assert correct(f, used, return_mask=True)[1].all() and not correct(f, L, return_mask=True)[1].all()


@pytest.mark.parametrize("dtype", LC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_raw_path(dev, dtype):
    """debayer(..., lens=) == correct(debayer(...), lens), plain and developed; debayer_frames_device(..., lens=) alike"""
    from shinestacker_amd import Cfa, Develop, debayer
    from shinestacker_amd.demosaic import debayer_frames_device, mosaic_of
    from shinestacker_amd.lens import correct
    shape = (33, 47)
    L = LC.lens_of("mixed", "off", shape)
    cfa = Cfa("GRBG", black=LC.maxv(dtype) // 32, gains=[1.9, 1.0, 1.0, 1.4])
    mosaics = [mosaic_of(LC.frame(k, shape, dtype), "GRBG") for k in ("random", "ramp")]
    plain = [debayer(m, cfa) for m in mosaics]
    for m, p in zip(mosaics, plain):
        assert_same("plain", debayer(m, cfa, lens=L), correct(p, L))
        assert_same("lens=None", debayer(m, cfa, lens=None), p)
    with Develop(matrix=[[1.4, -0.3, -0.1], [-0.2, 1.5, -0.3], [0.0, -0.4, 1.4]], tone="srgb") as d:
        want = correct(debayer(mosaics[0], cfa, develop=d), L)
        assert_same("developed", debayer(mosaics[0], cfa, develop=d, lens=L), want)
    fb = plain[0].nbytes
    out = dev.DeviceBuffer(2 * fb)
    try:
        debayer_frames_device(mosaics, out.ptr, cfa, lens=L)
        for i, p in enumerate(plain):
            assert_same(("frames", i), out.download(p.shape, dtype, i * fb), correct(p, L))
    finally:
        out.free()


def _moving_frames(oracle, n=6, h=64, w=96):
    """six frames of one texture with a small known motion"""
    from ecc_pairs import make_pair, similarity
    frames = []
    for f in range(n):
        d = f - n // 2
        T = similarity(0.05 * d, 1 + 3e-4 * d, 0.5 * d, -0.3 * d, (w - 1) / 2, (h - 1) / 2)
        ref, mov = make_pair(oracle, T, h=h, w=w, seed=11, noise=2.0)
        frames.append(ref if d == 0 else mov)
    return frames


def test_align_and_stack_with_a_lens(dev, oracle):
    """align_and_stack(frames, lens=L) == align_and_stack([correct(f, L) for f in frames])"""
    from shinestacker_amd.align import ecc_estimator
    from shinestacker_amd.lens import correct
    from shinestacker_amd.pipeline import align_and_stack
    frames = _moving_frames(oracle)
    L = LC.lens_of("mixed", "default", (64, 96))
    kw = dict(estimator=ecc_estimator(), alignment_config=dict(subsample=1), min_size=16, arith="exact")
    out, matches = align_and_stack(frames, lens=L, **kw)
    fixed = [correct(f, L) for f in frames]
    assert all((a != b).any() for a, b in zip(fixed, frames))
    out2, matches2 = align_and_stack(fixed, **kw)
    assert_same("host pipeline", out, out2)
    assert matches == matches2
    out3, _ = align_and_stack(frames, **kw)
    assert not np.array_equal(out, out3)
    assert_same("lens=None", align_and_stack(frames, lens=None, **kw)[0], out3)
    assert_same("options dict", align_and_stack(frames, lens={"lens": L}, **kw)[0], out)


def test_align_and_stack_device_with_a_lens(dev, oracle):
    """align_and_stack_device(..., lens=L) on a resident stack == the frames corrected one at a time, then the pipeline"""
    from shinestacker_amd.lens import correct
    from shinestacker_amd.pipeline import align_and_stack_device
    frames = _moving_frames(oracle)
    n, (h, w) = len(frames), frames[0].shape[:2]
    fb = frames[0].nbytes
    L = LC.lens_of("mixed", "default", (h, w))

    def resident(fs):
        buf = dev.DeviceBuffer(fb * n)
        for i, f in enumerate(fs):
            buf.upload(f, i * fb)
        return buf
    kw = dict(alignment_config=dict(subsample=1), min_size=16, arith="exact")
    fixed = [correct(f, L) for f in frames]
    buf = resident(frames)
    try:
        out, ms, ccs = align_and_stack_device(buf.ptr, n, h, w, np.uint8, lens=L, **kw)
        assert_same("corrected in place", buf.download((n,) + frames[0].shape, np.uint8), np.stack(fixed))
    finally:
        buf.free()
    buf = resident(fixed)
    try:
        out2, ms2, ccs2 = align_and_stack_device(buf.ptr, n, h, w, np.uint8, **kw)
    finally:
        buf.free()
    assert_same("device pipeline", out, out2)
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(ms, ms2)) and ccs == ccs2
    buf = resident(frames)
    try:
        a = align_and_stack_device(buf.ptr, n, h, w, np.uint8, **kw)
        b = align_and_stack_device(buf.ptr, n, h, w, np.uint8, lens=None, **kw)
        assert_same("untouched", buf.download((n,) + frames[0].shape, np.uint8), np.stack(frames))
    finally:
        buf.free()
    assert_same("lens=None", a[0], b[0])
    assert not np.array_equal(a[0], out)


@pytest.mark.parametrize("step_process", [False, True], ids=["fixed-reference", "step_process"])
def test_combined_actions_job_on_files(dev, oracle, tmp_path, step_process):
    """CombinedActions([LensCorrection, AlignFrames]) on files == CombinedActions([AlignFrames]) on the frames corrected by hand:
    the reference frame AlignFrames fits to has passed the lens correction too (CombinedActions.img_ref), not only the frame
    being processed"""
    import os
    from shinestacker_amd import AlignFrames, CombinedActions, LensCorrection, StackJob
    from shinestacker_amd.align import ecc_estimator
    from shinestacker_amd.imageio import read_img, write_img
    from shinestacker_amd.lens import correct
    frames = _moving_frames(oracle)
    L = LC.lens_of("mixed", "default", frames[0].shape[:2])
    fixed = [correct(f, L) for f in frames]
    work = str(tmp_path)
    names = [f"f{i:02d}.png" for i in range(len(frames))]
    for sub, fs in (("raw", frames), ("fixed", fixed)):
        os.makedirs(os.path.join(work, sub))
        for n, f in zip(names, fs):
            write_img(os.path.join(work, sub, n), f)
    assert np.array_equal(read_img(os.path.join(work, "fixed", names[0])), fixed[0])       # (the files are lossless)

    def align():
        return AlignFrames(estimator=ecc_estimator(), subsample=1)
    job = StackJob("job", work, input_path="raw")
    job.add_action(CombinedActions("with-lens", [LensCorrection(L), align()], input_path="raw", output_path="out-lens",
                                   step_process=step_process))
    job.add_action(CombinedActions("by-hand", [align()], input_path="fixed", output_path="out-hand", step_process=step_process))
    job.add_action(CombinedActions("no-lens", [align()], input_path="raw", output_path="out-raw", step_process=step_process))
    job.run()
    ref = len(names) // 2
    for i, n in enumerate(names):
        got, want = read_img(os.path.join(work, "out-lens", n)), read_img(os.path.join(work, "out-hand", n))
        assert_same(("job", step_process, n), got, want)
        assert not np.array_equal(got, read_img(os.path.join(work, "out-raw", n))), n
        if i == ref:
            assert_same("the reference frame is written corrected", got, fixed[ref])


def test_overflowing_coefficients(dev):
    """coefficients at the end of the float64 range: inf and NaN on the way to the position; the kernel's min / max treat a NaN
    as the restatement's np.fmin / np.fmax do"""
    import lens_restatement as R
    from shinestacker_amd import Lens
    from shinestacker_amd.lens import correct
    for shape in ((33, 47), (16, 64)):
        for dtype in LC.DTYPES:
            f = LC.frame("random", shape, dtype)
            for name, k in LC.OVERFLOWING.items():
                for c in (None, LC.centre("off", shape)):
                    want, want_mask = R.remap(f, k, c, return_mask=True)
                    got, mask = correct(f, Lens(k, c), return_mask=True)
                    assert_same((shape, name, c), got, want)
                    assert_same((shape, name, c, "the mask"), mask, want_mask)
