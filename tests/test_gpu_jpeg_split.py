"""GPU: the split JPEG decoder (csrc/kernels_jpeg_split.hpp) equals its restatement (tests/jpeg_split_restatement.py) bit for
bit on the cases of tests/jpeg_split_cases.py -- files without a restart interval, with one above jpeg.MAX_DRI, short and
corrupt streams in one piece, and files with intervals sent there by split="always" -- coefficients, status words and
frames, at 8, 16 and 128 bytes a subsequence, in host form and in device form; the frames equal Pillow's where a codec is
specified on the case; with one round where the dense pictures need more the device form says so and the host form and
jpeg.Pusher repair it; and the layers above (PyramidStack / DepthMapStack(jpeg=, jpeg_split=True), jpeg.frames_device(split=))
equal the same call on the frames the host decodes.  Every comparison is array_equal."""
import io
import os

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_restatement as R
import jpeg_split_cases as SC
import jpeg_split_restatement as S
from shinestacker_amd import jpeg
from shinestacker_amd.errors import ImageLoadError, InvalidOptionError

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of the device buffer the kernels write
NEEDED = SC.PLAIN + SC.LONG + [s[0] for s in SC.SHORT]


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


def _pillow(data):
    try:
        from PIL import Image
    except ImportError:
        return None
    a = np.array(Image.open(io.BytesIO(data)))
    return np.repeat(a[:, :, None], 3, 2) if a.ndim == 2 else np.ascontiguousarray(a[:, :, ::-1])


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{case name: (path, the restated coefficient planes, status words, BGR frame, Pillow's frame or None)}: written and
    restated once"""
    d = tmp_path_factory.mktemp("jpeg_split")
    out = {}
    for c in NEEDED + SC.ALWAYS:
        path = c.write(str(d / (c.name + ".jpg")))
        h = R.parse(c.data())
        planes, status = S.walk_split(c.data(), h)
        bgr = R.render(planes, h)
        pil = _pillow(c.data()) if c.codec else None
        for a in planes + [status, bgr]:
            a.setflags(write=False)
        out[c.name] = (path, planes, status, bgr, pil)
    return out


def _frame(table, case, sub=0, rounds=0):
    f = jpeg.read(table[case.name][0], split="always" if case in SC.ALWAYS else "needed")
    assert f.split
    f.split_options = (sub, rounds)
    return f


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


@pytest.mark.parametrize("sub", [8, 16, 128])
def test_coefficients_and_status_equal_the_restatement(dev, table, sub):
    flagged = 0
    for c in NEEDED + SC.ALWAYS:
        _, planes, status, _, _ = table[c.name]
        got, st = jpeg.coefficients(_frame(table, c, sub))
        assert_same((c.name, "status"), st, status)
        assert len(got) == len(planes)
        for k, (g, w) in enumerate(zip(got, planes)):
            assert_same((c.name, k), g, w)
        flagged += bool(status.any())
    assert flagged == len(SC.SHORT)


def test_decode_equals_the_restatement_and_pillow(dev, table):
    with_codec = 0
    for c in NEEDED + SC.ALWAYS:
        _, _, status, bgr, pil = table[c.name]
        frame = _frame(table, c)
        got, st = jpeg.decode(frame, status=True)
        assert_same((c.name, "status"), st, status)
        assert_same(c.name, got, bgr)
        if status.any():
            with pytest.raises(ImageLoadError, match="restart interval"):
                jpeg.decode(frame)
        if pil is not None:
            assert_same((c.name, "pillow"), got, pil)
            with_codec += 1
    try:
        import PIL  # noqa: F401
        assert with_codec >= len(SC.PLAIN) - 2
    except ImportError:
        pass


@pytest.mark.parametrize("stream", ["null-stream", "side-stream"])
def test_decode_device_equals_the_restatement(dev, side, table, stream):
    slot = jpeg.Slot(0)
    try:
        for c in NEEDED + SC.ALWAYS[:2]:
            _, _, status, bgr, _ = table[c.name]
            frame = _frame(table, c, 16 if stream == "side-stream" else 0)
            out = dev.DeviceBuffer(bgr.nbytes + 2 * GUARD)
            try:
                out.upload(np.full(out.nbytes, 0xA5, np.uint8))
                assert jpeg.decode_device(frame, out.ptr + GUARD, slot, 0, side.stream if stream == "side-stream" else None) is slot
                if stream == "side-stream":
                    side.sync()
                else:
                    dev.check(dev.load().mi_device_synchronize(0))
                raw = out.download((out.nbytes,), np.uint8)
                assert_same((c.name, "status"), slot.status(), status)
            finally:
                out.free()
            assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), c.name
            assert_same(c.name, raw[GUARD:-GUARD].reshape(bgr.shape), bgr)
    finally:
        slot.free()


def test_too_few_rounds_are_reported_and_repaired(dev, table):
    """8 bytes a subsequence and ONE round across groups on the dense pictures, which need four or five
    (tests/test_jpeg_split_host.py): the device form reports UNSYNCED and nothing else; the host form and jpeg.Pusher decode
    again with every round and return the exact frame"""
    by_name = {c.name: c for c in SC.PLAIN}
    for name in SC.SLOW:
        c = by_name[name]
        _, planes, status, bgr, _ = table[name]
        assert not status.any()
        frame = _frame(table, c, 8, 1)
        out = dev.DeviceBuffer(bgr.nbytes)
        try:
            slot = jpeg.decode_device(frame, out.ptr)
            dev.check(dev.load().mi_device_synchronize(0))
            assert slot.status().tolist() == [dev.JPEG_UNSYNCED], name
            assert_same((name, "settled"), jpeg.settle(frame, out.ptr, slot), status)
            assert_same((name, "settled frame"), out.download(bgr.shape, np.uint8), bgr)
            slot.free()
        finally:
            out.free()
        got, st = jpeg.decode(frame, status=True)
        assert_same((name, "host status"), st, status)
        assert_same((name, "host"), got, bgr)
        coef, st = jpeg.coefficients(frame)
        assert not st.any()
        for k, (g, w) in enumerate(zip(coef, planes)):
            assert_same((name, k), g, w)
        pusher, seen = jpeg.Pusher(0), []
        try:
            pusher.push(frame, lambda ptr: seen.append((ptr == pusher.bgr[0].ptr, pusher.bgr[0].download(bgr.shape, np.uint8))), lambda: None)
        finally:
            pusher.close()
        assert len(seen) == 1 and seen[0][0]
        assert_same((name, "pusher"), seen[0][1], bgr)


def test_files_with_intervals_through_always_equal_the_serial_path(dev, table):
    for c in SC.ALWAYS:
        path = table[c.name][0]
        a, b = jpeg.read(path), jpeg.read(path, split="always")
        assert not a.split and b.split and a.n_intervals == b.n_intervals > 1
        (ca, sa), (cb, sb) = jpeg.coefficients(a), jpeg.coefficients(b)
        assert_same((c.name, "status"), sb, sa)
        for k, (x, y) in enumerate(zip(ca, cb)):
            assert_same((c.name, k), y, x)
        assert_same(c.name, jpeg.decode(b), jpeg.decode(a))


class _Quiet:
    """the little of an action a stacker talks to"""
    id, name = 0, "quiet"

    def sub_message_r(self, *a, **k):
        pass

    def callback(self, *a, **k):
        return None


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """six 37 x 53 files, with and without restart intervals in alternation, one of them with DRI 8193, and the frames Pillow
    decodes from them; and a progressive file, which stays refused"""
    pytest.importorskip("PIL")
    from shinestacker_amd import imageio
    if imageio._cv2 is not None:
        pytest.skip("the host decoder is OpenCV: its JPEG decoder is not the one the statement is pinned against")
    d = tmp_path_factory.mktemp("folder")
    paths = []
    for i, mode in enumerate(("444", "420", "422", "444", "420", "grey")):
        p = str(d / f"f{i}.jpg")
        with open(p, "wb") as fh:
            fh.write(JC.write(37, 53, mode=mode, dri=(0, 3, 0, 8193, 2, 0)[i], seed=300 + i, quality=("mid", "fine")[i & 1]))
        paths.append(p)
    host = [imageio.read_img(p) for p in paths]
    assert all(f is not None and f.shape == (37, 53, 3) for f in host)
    progressive = str(d / "progressive.jpg")
    from PIL import Image
    Image.fromarray(JC.picture(37, 53, 9)).save(progressive, "JPEG", progressive=True)
    return paths, host, progressive


def _stackers():
    from shinestacker_amd import DepthMapStack, PyramidStack
    return (("pyramid", lambda **kw: PyramidStack(min_size=8, **kw)), ("depth-map", lambda **kw: DepthMapStack(**kw)))


@pytest.mark.parametrize("which", [0, 1], ids=["pyramid", "depth-map"])
def test_stackers_decode_plain_files_on_the_device(dev, folder, which):
    paths, host, progressive = folder
    _, make = _stackers()[which]
    a, b, c, d = make(), make(jpeg="device", jpeg_split=True), make(jpeg="auto", jpeg_split=True), make(jpeg="auto")
    try:
        a.process = b.process = c.process = d.process = _Quiet()
        want = a.focus_stack(paths)
        assert_same("arrays", want, a.focus_stack_arrays(host))
        assert_same("device", b.focus_stack(paths), want)
        assert b.skipped == []
        assert_same("again", b.focus_stack(paths[:4]), a.focus_stack(paths[:4]))      # the stacker is reused
        # a file still refused falls back under "auto" exactly as before, and raises under "device"
        mixed = paths[:3] + [progressive] + paths[3:]
        assert_same("auto", c.focus_stack(mixed), a.focus_stack(mixed))
        assert [p for p, _ in c.skipped] == [progressive] and "SOF2 (progressive DCT)" in c.skipped[0][1]
        with pytest.raises(InvalidOptionError, match="SOF2"):
            b.focus_stack(mixed)
        # with jpeg_split at its default nothing changes: the plain files are refused with the text they always had
        assert_same("default", d.focus_stack(paths), want)
        assert [p for p, _ in d.skipped] == [paths[0], paths[2], paths[3], paths[5]]
        assert "DRI = none: " in d.skipped[0][1] and "no restart interval: the scan is one serial walk" in d.skipped[0][1]
        assert "DRI = 8193: " in d.skipped[2][1]
        e = make(jpeg="device")
        try:
            e.process = _Quiet()
            with pytest.raises(InvalidOptionError, match="DRI = none"):
                e.focus_stack(paths)
        finally:
            e.close()
    finally:
        for s in (a, b, c, d):
            s.close()


def test_frames_device_feeds_the_resident_pipeline(dev, folder):
    from shinestacker_amd import pipeline
    paths, host, progressive = folder
    n, (h, w) = len(paths), host[0].shape[:2]
    fb = h * w * 3
    mine, theirs = dev.DeviceBuffer(n * fb), dev.DeviceBuffer(n * fb)
    try:
        assert jpeg.frames_device(paths, mine.ptr, split="needed") == (h, w, np.dtype(np.uint8))
        for i in range(n):
            assert_same(("frame", i), mine.download((h, w, 3), np.uint8, i * fb), host[i])
        theirs.upload(np.stack(host))
        got = pipeline.align_and_stack_device(mine.ptr, n, h, w, np.uint8, min_size=8)
        want = pipeline.align_and_stack_device(theirs.ptr, n, h, w, np.uint8, min_size=8)
        assert_same("fused", got[0], want[0])
        assert jpeg.frames_device(paths, mine.ptr, split="always") == (h, w, np.dtype(np.uint8))
        for i in range(n):
            assert_same(("always", i), mine.download((h, w, 3), np.uint8, i * fb), host[i])
        with pytest.raises(InvalidOptionError, match="DRI = none"):
            jpeg.frames_device(paths, mine.ptr)
        with pytest.raises(InvalidOptionError, match="SOF2"):
            jpeg.frames_device(paths[:1] + [progressive], mine.ptr, split="needed")
    finally:
        mine.free()
        theirs.free()
