"""GPU: the JPEG kernels (csrc/kernels_jpeg.hpp) equal their restatement (tests/jpeg_restatement.py) bit for bit on the cases
of tests/jpeg_cases.py -- which the CPU tests show to be meaningful and pin against libjpeg-turbo -- coefficients, status
words and frames, in host form and in device form, the flagged streams included (they are the walker's defined behaviour,
and the CPU program has run them under the sanitizers); and the layers above (PyramidStack(jpeg=), DepthMapStack(jpeg=),
jpeg.frames_device) equal the same call on the frames the host decodes.  Every comparison is array_equal.

jpeg.frames_device is compared through pipeline.align_and_stack_device on both sides -- its own buffer against a buffer of
host-decoded frames -- not against pipeline.align_and_stack: the host pipeline runs another estimator, so the two differ by
more than this decoder could account for."""
import os

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_restatement as R
from shinestacker_amd import jpeg
from shinestacker_amd.errors import ImageLoadError, InvalidOptionError

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of the device buffer the kernels write
ALL = JC.CASES + [s[0] for s in JC.SHORT]


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
    """{case name: (JpegFrame, the restated coefficient planes, status words, BGR frame)}: written, parsed, restated once"""
    d = tmp_path_factory.mktemp("jpeg")
    out = {}
    for c in ALL:
        frame = jpeg.read(c.write(str(d / (c.name + ".jpg"))))
        h = R.parse(c.data())
        planes, status = R.walk(c.data(), h)
        bgr = R.render(planes, h)
        for a in planes + [status, bgr]:
            a.setflags(write=False)
        out[c.name] = (frame, planes, status, bgr)
    return out


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def test_coefficients_and_status_equal_the_restatement(dev, table):
    flagged = 0
    for name, (frame, planes, status, _) in table.items():
        got, st = jpeg.coefficients(frame)
        assert_same((name, "status"), st, status)
        assert len(got) == len(planes)
        for c, (g, w) in enumerate(zip(got, planes)):
            assert_same((name, c), g, w)
        flagged += bool(status.any())
    assert flagged == len(JC.SHORT)


def test_decode_equals_the_restatement(dev, table):
    for name, (frame, _, status, bgr) in table.items():
        got, st = jpeg.decode(frame, status=True)
        assert_same((name, "status"), st, status)
        assert_same(name, got, bgr)
        if status.any():
            with pytest.raises(ImageLoadError, match="restart interval"):
                jpeg.decode(frame)
        else:
            assert_same(name, jpeg.decode(frame), bgr)


@pytest.mark.parametrize("stream", ["null-stream", "side-stream"])
def test_decode_device_equals_the_restatement(dev, side, table, stream):
    slot = jpeg.Slot(0)
    try:
        for name, (frame, _, status, bgr) in table.items():
            out = dev.DeviceBuffer(bgr.nbytes + 2 * GUARD)
            try:
                out.upload(np.full(out.nbytes, 0xA5, np.uint8))
                assert jpeg.decode_device(frame, out.ptr + GUARD, slot, 0, side.stream if stream == "side-stream" else None) is slot
                if stream == "side-stream":
                    side.sync()
                else:
                    dev.check(dev.load().mi_device_synchronize(0))
                raw = out.download((out.nbytes,), np.uint8)
                assert_same((name, "status"), slot.status(), status)
            finally:
                out.free()
            assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), name
            assert_same(name, raw[GUARD:-GUARD].reshape(bgr.shape), bgr)
    finally:
        slot.free()


class _Quiet:
    """the little of an action a stacker talks to"""
    id, name = 0, "quiet"

    def sub_message_r(self, *a, **k):
        pass

    def callback(self, *a, **k):
        return None


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """six 37 x 53 files with restart intervals, one mode after the other, and the frames Pillow decodes from them"""
    pytest.importorskip("PIL")
    from shinestacker_amd import imageio
    if imageio._cv2 is not None:
        pytest.skip("the host decoder is OpenCV: its JPEG decoder is not the one the statement is pinned against")
    d = tmp_path_factory.mktemp("folder")
    paths = []
    for i, mode in enumerate(("444", "420", "422", "444", "420", "grey")):
        p = str(d / f"f{i}.jpg")
        with open(p, "wb") as fh:
            fh.write(JC.write(37, 53, mode=mode, dri=(1, 3, 4, 7, 2, 5)[i], seed=100 + i, quality=("mid", "fine")[i & 1]))
        paths.append(p)
    host = [imageio.read_img(p) for p in paths]
    assert all(f is not None and f.shape == (37, 53, 3) for f in host)
    plain = str(d / "plain.jpg")          # no restart interval: what jpeg.read refuses
    with open(plain, "wb") as fh:
        fh.write(JC.write(37, 53, mode="420", dri=0, seed=200))
    cut = str(d / "cut.jpg")              # an interval that ends early
    with open(cut, "wb") as fh:
        fh.write(JC.write(37, 53, mode="420", dri=4, seed=21, tweak={"truncate": 1}))
    return paths, host, plain, cut


def _stackers():
    from shinestacker_amd import DepthMapStack, PyramidStack
    return (("pyramid", lambda **kw: PyramidStack(min_size=8, **kw)), ("depth-map", lambda **kw: DepthMapStack(**kw)))


@pytest.mark.parametrize("which", [0, 1], ids=["pyramid", "depth-map"])
@pytest.mark.parametrize("threads", [1, 8])
def test_stackers_decode_on_the_device(dev, folder, which, threads):
    paths, host, _, _ = folder
    _, make = _stackers()[which]
    a, b = make(decode_threads=threads), make(jpeg="device", decode_threads=threads)
    try:
        a.process = b.process = _Quiet()
        want = a.focus_stack(paths)
        assert_same("arrays", want, a.focus_stack_arrays(host))
        got = b.focus_stack(paths)
        assert_same("device", got, want)
        assert b.skipped == []
        assert_same("again", b.focus_stack(paths[:4]), a.focus_stack(paths[:4]))      # the stacker is reused
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("which", [0, 1], ids=["pyramid", "depth-map"])
def test_auto_falls_back_and_device_refuses(dev, folder, which):
    paths, _, plain, cut = folder
    _, make = _stackers()[which]
    mixed = paths[:2] + [plain] + paths[2:4]
    a, b, c = make(), make(jpeg="auto"), make(jpeg="device")
    try:
        a.process = b.process = c.process = _Quiet()
        assert_same("auto", b.focus_stack(mixed), a.focus_stack(mixed))
        assert [p for p, _ in b.skipped] == [plain] and "DRI = none" in b.skipped[0][1]
        # several refused files: each once, in file order, whatever order the pool finished them in; and a file that was
        # read ahead of an earlier error never reached the stack, so it is not listed
        plain2 = os.path.join(os.path.dirname(plain), "plain2.jpg")
        with open(plain2, "wb") as fh:
            fh.write(JC.write(37, 53, mode="444", dri=0, seed=201))
        many = [plain2, paths[0], plain, paths[1], plain2]
        for threads in (1, 8):
            b.decode_threads = a.decode_threads = threads
            assert_same(("auto", threads), b.focus_stack(many), a.focus_stack(many))
            assert [p for p, _ in b.skipped] == [plain2, plain, plain2]
            with pytest.raises(ImageLoadError):
                b.focus_stack([paths[0], cut, plain, plain2])
            assert b.skipped == []
        with pytest.raises(InvalidOptionError, match="DRI = none"):
            c.focus_stack(mixed)
        # a file that decodes with a status flag raises under both
        for algo in (b, c):
            with pytest.raises(ImageLoadError) as e:
                algo.focus_stack(paths[:2] + [cut])
            assert cut in str(e.value) and "the data ended" in str(e.value) and "status 2" in str(e.value)
        assert_same("after an error", c.focus_stack(paths), a.focus_stack(paths))
        # shape validation is the host path's
        other = os.path.join(os.path.dirname(plain), "other.jpg")
        with open(other, "wb") as fh:
            fh.write(JC.write(31, 15, mode="444", dri=1, seed=3))
        from shinestacker_amd.errors import ShapeError
        for algo in (a, c):
            with pytest.raises(ShapeError):
                algo.focus_stack(paths[:2] + [other])
    finally:
        for s in (a, b, c):
            s.close()


def test_frames_device_feeds_the_resident_pipeline(dev, folder):
    from shinestacker_amd import pipeline
    paths, host, plain, cut = folder
    n, (h, w) = len(paths), host[0].shape[:2]
    fb = h * w * 3
    mine, theirs = dev.DeviceBuffer(n * fb), dev.DeviceBuffer(n * fb)
    try:
        assert jpeg.frames_device(paths, mine.ptr) == (h, w, np.dtype(np.uint8))
        for i in range(n):
            assert_same(("frame", i), mine.download((h, w, 3), np.uint8, i * fb), host[i])
        theirs.upload(np.stack(host))
        got = pipeline.align_and_stack_device(mine.ptr, n, h, w, np.uint8, min_size=8)
        want = pipeline.align_and_stack_device(theirs.ptr, n, h, w, np.uint8, min_size=8)
        assert_same("fused", got[0], want[0])
        with pytest.raises(InvalidOptionError, match="DRI = none"):
            jpeg.frames_device(paths[:1] + [plain], mine.ptr)
        with pytest.raises(ImageLoadError, match="status 2"):
            jpeg.frames_device(paths[:3] + [cut], mine.ptr)
    finally:
        mine.free()
        theirs.free()
