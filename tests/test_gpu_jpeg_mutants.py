"""GPU: jpeg_entropy, the split JPEG kernels, jpeg_idct and jpeg_colour on the seeded corrupt files of tests/jpeg_mutants.py that
jpeg.read accepts.

What runs is jpeg_mutants.device_selection(): at most 300 accepted mutants, no two with the same headers and scan bytes, which
test_jpeg_mutants_host.py shows to hold, for each of 4:4:4, 4:2:2, 4:2:0 and grey and for files with and without restart
intervals, a mutant with status 0 and other coefficients than its base, one with bits that match no code, one whose data ends
early, one whose run passes coefficient 63, a moved Huffman code that still decodes, a changed quantisation entry and an EOI
in the middle of an interval -- and changed sizes, selectors, DRI values and tables that jpeg.read still accepted.  Every one
has gone through the plain C++ cores on the CPU under sanitizers first (test_jpeg_core_host.py, test_jpeg_split_core_host.py)
and equalled its restatement there.  These are inputs whose complete output the kernels' contract defines ("a corrupt stream
costs a status bit and nothing else"); none is chosen to make anything fall over.

    serial path    the mutants read with their restart intervals (split=None): mi_jpeg_coefficients[_device] and
                   mi_jpeg_decode[_device] -- status words and int16 coefficient planes equal jpeg_restatement.walk, flagged
                   intervals included, and the BGR frame equals render of those coefficients over the whole picture
    split path     every mutant (split="always"): mi_jpeg_split_coefficients[_device] and mi_jpeg_split_decode[_device] at 8, 16
                   and 128 bytes a subsequence, the device forms with every round -- status words and coefficients equal
                   jpeg_split_restatement.walk_split (unreached coefficients and DC differences are 0: equality, not a
                   subset), the frame equals render, no word carries MI_JPEG_UNSYNCED
    device forms   between 256-byte guard bands of 0xA5, on the null stream and on a handle's stream
    the boundary   the host forms go through the C boundary's argument checks: a refusal of what jpeg.read accepted fails here
    a short span   bases with span_bytes DECLARED shorter than the buffer, at three seeded cut points: both paths
    one level up   ten mutants with a status that is not 0: jpeg.decode, jpeg.frames_device, jpeg.Pusher and PyramidStack under
                   jpeg="device" AND under "auto" raise ImageLoadError naming the file, the interval and the status ("auto"
                   falls back to the host only for what jpeg.read REFUSES), and the Pusher and the stacker that met them
                   then give what fresh ones give

Everything is array_equal.

Time, measured on the MI355X machine: the `selection` fixture -- the corpus written and parsed (23 912 small files, three
reads each, host Python), the class search (at most 12 restatements a base) and the 300 restatements with their renders --
takes 12 s, once (32 s on a slower, busier CPU; the DNG corpus takes 7 to 8 s on the same machine); every test then takes 0.1
to 0.45 s (165 mutants on the serial path, 300 on the split path: some 5 000 launches in all) and the whole file 17.5 s.
"""
import copy

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_mutants as M
import jpeg_restatement as R
import jpeg_split_restatement as S
from shinestacker_amd import jpeg
from shinestacker_amd.errors import ImageLoadError

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of the device buffer the kernels write
SUBS = (8, 16, 128)


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
def selection():
    sel = M.device_selection()
    assert len(sel) <= M.DEVICE_LIMIT and len({o.key() for o in sel}) == len(sel)
    for o in sel:
        r = M.restated(o)
        r.bgr("split")
        if r.serial is not None:
            r.bgr("serial")
    assert sum(o.serial for o in sel) >= 100 and sum(not o.serial for o in sel) >= 100
    return sel


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def frame_of(outcome, split, sub=0, rounds=0):
    """the frame jpeg.read returned at `split` (None or "always"), a copy with its own split options"""
    f = copy.copy(outcome.frames[split])
    assert f.split == (split == "always")
    f.split_options = (sub, rounds)
    return f


def flat(planes):
    return np.concatenate([p.reshape(-1) for p in planes])


def wait(dev, side, stream):
    if stream:
        side.sync()
    else:
        dev.check(dev.load().mi_device_synchronize(0))


def guarded(dev, nbytes):
    out = dev.DeviceBuffer(nbytes + 2 * GUARD)
    out.upload(np.full(out.nbytes, 0xA5, np.uint8))
    return out


def unguarded(out, nbytes, dtype, name):
    raw = out.download((out.nbytes,), np.uint8)
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + nbytes:] == 0xA5).all(), (name, "the guard band around the output was written")
    return raw[GUARD:GUARD + nbytes].copy().view(dtype)


def device_forms(dev, side, slot, frame, stream, name, span_bytes=None):
    """(coefficients, their status words, the BGR frame, its status words) of the frame's two device forms, each output
    between guard bands; the split decoder is given every round.  span_bytes: the span is declared that long."""
    lib, C = dev.load(), dev.C
    slot.load(frame)
    nbytes = slot.span_bytes if span_bytes is None else span_bytes
    n = C.c_size_t()
    dev.check(lib.mi_jpeg_coef_count(C.byref(frame.desc), C.byref(n)))
    h, w = frame.shape
    opt = dev.JpegSplitStruct(frame.split_options[0], dev.JPEG_SPLIT_ALL_ROUNDS)
    stale = np.full(frame.n_intervals, 0xFFFFFFFF, np.uint32)
    coef, bgr = guarded(dev, 2 * n.value), guarded(dev, h * w * 3)
    try:
        slot.buf.upload(stale, slot.status_at)
        if frame.split:
            dev.check(lib.mi_jpeg_split_coefficients_device(0, stream, slot.buf.ptr, nbytes, slot.buf.ptr + slot.off_at, C.byref(frame.desc),
                                                            C.byref(opt), slot.scratch.ptr, slot.scratch.nbytes, coef.ptr + GUARD,
                                                            slot.buf.ptr + slot.status_at))
        else:
            dev.check(lib.mi_jpeg_coefficients_device(0, stream, slot.buf.ptr, nbytes, slot.buf.ptr + slot.off_at, C.byref(frame.desc),
                                                      coef.ptr + GUARD, slot.buf.ptr + slot.status_at))
        wait(dev, side, stream)
        st_coef = slot.status()
        got_coef = unguarded(coef, 2 * n.value, np.int16, name)
        slot.buf.upload(stale, slot.status_at)
        if frame.split:
            dev.check(lib.mi_jpeg_split_decode_device(0, stream, slot.buf.ptr, nbytes, slot.buf.ptr + slot.off_at, C.byref(frame.desc),
                                                      C.byref(opt), slot.scratch.ptr, slot.scratch.nbytes, bgr.ptr + GUARD,
                                                      slot.buf.ptr + slot.status_at))
        else:
            dev.check(lib.mi_jpeg_decode_device(0, stream, slot.buf.ptr, nbytes, slot.buf.ptr + slot.off_at, C.byref(frame.desc),
                                                slot.scratch.ptr, slot.scratch.nbytes, bgr.ptr + GUARD, slot.buf.ptr + slot.status_at))
        wait(dev, side, stream)
        st_bgr = slot.status()
        got_bgr = unguarded(bgr, h * w * 3, np.uint8, name).reshape(h, w, 3)
    finally:
        coef.free()
        bgr.free()
    return got_coef, st_coef, got_bgr, st_bgr


def check_device(dev, side, slot, frame, stream, name, planes, status, bgr, span_bytes=None):
    got_coef, st_coef, got_bgr, st_bgr = device_forms(dev, side, slot, frame, stream, name, span_bytes)
    assert not ((st_coef | st_bgr) & dev.JPEG_UNSYNCED).any(), (name, st_coef.tolist(), st_bgr.tolist())
    assert_same((name, "coefficient status"), st_coef, status)
    assert_same((name, "coefficients"), got_coef, flat(planes))
    assert_same((name, "decode status"), st_bgr, status)
    assert_same((name, "frame"), got_bgr, bgr)


def check_host(frame, name, planes, status, bgr):
    """jpeg.coefficients and jpeg.decode: the host forms, argument checks included (a refusal raises DeviceError)"""
    got, st = jpeg.coefficients(frame)
    assert_same((name, "coefficient status"), st, status)
    assert len(got) == len(planes), name
    for k, (g, w) in enumerate(zip(got, planes)):
        assert_same((name, "coefficients", k), g, w)
    out, st = jpeg.decode(frame, status=True)
    assert_same((name, "decode status"), st, status)
    assert_same((name, "frame"), out, bgr)


def flags_of(status_words):
    out = set()
    for status in status_words:
        out |= {"clean"} if not status.any() else set()
        for name, bit in (("nocode", M.NOCODE), ("overrun", M.OVERRUN), ("run", M.RUN)):
            out |= {name} if (status & bit).any() else set()
    return out


ALL_FLAGS = {"clean", "nocode", "overrun", "run"}


def test_the_serial_host_forms_equal_the_restatement_on_the_mutants(dev, selection):
    mine = [o for o in selection if o.serial]
    assert flags_of(M.restated(o).serial[1] for o in mine) == ALL_FLAGS
    for o in mine:
        r = M.restated(o)
        check_host(frame_of(o, None), o.recipe, *r.serial, r.bgr("serial"))


@pytest.mark.parametrize("stream", ["null-stream", "side-stream"])
def test_the_serial_device_forms_equal_the_restatement_on_the_mutants(dev, side, selection, stream):
    slot = jpeg.Slot(0)
    try:
        for o in selection:
            if o.serial:
                r = M.restated(o)
                check_device(dev, side, slot, frame_of(o, None), side.stream if stream == "side-stream" else None, o.recipe,
                             *r.serial, r.bgr("serial"))
    finally:
        slot.free()


@pytest.mark.parametrize("sub", SUBS)
def test_the_split_host_forms_equal_the_restatement_on_the_mutants(dev, selection, sub):
    assert flags_of(M.restated(o).split[1] for o in selection) == ALL_FLAGS
    for o in selection:
        r = M.restated(o)
        check_host(frame_of(o, "always", sub), (o.recipe, sub), *r.split, r.bgr("split"))


@pytest.mark.parametrize("stream", ["null-stream", "side-stream"])
@pytest.mark.parametrize("sub", SUBS)
def test_the_split_device_forms_equal_the_restatement_on_the_mutants(dev, side, selection, sub, stream):
    slot = jpeg.Slot(0)
    try:
        for o in selection:
            r = M.restated(o)
            check_device(dev, side, slot, frame_of(o, "always", sub), side.stream if stream == "side-stream" else None, (o.recipe, sub),
                         *r.split, r.bgr("split"))
    finally:
        slot.free()


SHORT_BASES = ("cases/37x53-420-dri5", "cases/37x53-444-dri3", "cases/17x33-422-row", "cases/31x15-grey-row", "plain/37x53-420",
               "plain/17x33-444", "plain/31x15-grey", "long/17x33-420-dri8193")


def test_a_span_declared_short_reads_nothing_beyond_it(dev, side):
    """the unmutated bases of SHORT_BASES with span_bytes DECLARED shorter than the buffer that holds the span, at three seeded
    cut points inside the scan: bytes at or beyond span_bytes count as absent, as the restatements cut the data there.  The
    serial path for the files with restart intervals, the split path (8 and 128 bytes a subsequence) for all."""
    slot, ran = jpeg.Slot(0), 0
    try:
        for name in SHORT_BASES:
            b = M.base(name)
            o = M.base_outcome(b)
            h = R.parse(b.data)
            rng = np.random.default_rng([b.index, 211])
            for short in sorted(int(v) for v in rng.integers(1, o.frame.span.nbytes, size=3)):
                cut = b.data[:h["scan_off"] + short]
                if o.serial:
                    planes, status = R.walk(cut, h)
                    assert status.any(), (name, short)
                    check_device(dev, side, slot, frame_of(o, None), None, (name, short), planes, status, R.render(planes, h), span_bytes=short)
                    ran += 1
                planes, status = S.walk_split(cut, h)
                assert status.any(), (name, short)
                for sub in (8, 128):
                    check_device(dev, side, slot, frame_of(o, "always", sub), side.stream, (name, short, sub), planes, status,
                                 R.render(planes, h), span_bytes=short)
                    ran += 1
    finally:
        slot.free()
    assert ran == 3 * (4 + 2 * len(SHORT_BASES))


# ---------------------------------------------------------------------------------------------- one level up
H, W = 37, 53


class _Quiet:
    """the little of an action a stacker talks to"""
    id, name = 0, "quiet"

    def sub_message_r(self, *a, **k):
        pass

    def callback(self, *a, **k):
        return None


@pytest.fixture(scope="module")
def stack_files(tmp_path_factory):
    """(three good 37 x 53 files -- 4:2:0 with DRI 3, 4:4:4 without DRI, 4:2:2 with DRI 5 -- and ten mutants of the first two,
    five each, whose restated status is not 0: [(path, split mode, the first flagged interval, its status)])"""
    d = tmp_path_factory.mktemp("mutant-stack")
    good = []
    for i, (mode, dri) in enumerate((("420", 3), ("444", 0), ("422", 5))):
        p = str(d / f"good{i}.jpg")
        with open(p, "wb") as fh:
            fh.write(JC.write(H, W, mode=mode, dri=dri, seed=400 + i))
        good.append(p)
    bad = []
    for i in (0, 1):
        with open(good[i], "rb") as fh:
            b = M.Base(f"stack/good{i}", fh.read())
        b.index = len(M.bases()) + i
        mine, early = [], 0
        for m in M.scan_mutants(b):
            o = M.parse(b, m)
            if len(mine) == 5 or not o.accepted:
                continue
            status = M.restated(o).native[1]
            only_early = not (status & (M.NOCODE | M.RUN)).any()
            if status.any() and (not only_early or early < 2):      # (data that ends early is the common one: two at the most)
                early += only_early
                p = str(d / f"bad{i}-{len(mine)}.jpg")
                with open(p, "wb") as fh:
                    fh.write(m.data)
                k = int(np.flatnonzero(status)[0])
                mine.append((p, None if o.serial else "needed", k, int(status[k]), len(status)))
        assert len(mine) == 5, (i, len(mine))
        bad += mine
    return good, bad


def _stacker(**kw):
    from shinestacker_amd import PyramidStack
    s = PyramidStack(min_size=8, **kw)
    s.process = _Quiet()
    return s


def _names(path, k, n, status):
    return [path, f"restart interval {k} of {n} ", f"status {status}:"]


def test_a_flagged_mutant_is_reported_and_the_pusher_and_the_stacker_go_on(dev, stack_files):
    """What jpeg="auto" does with a file jpeg.read accepts whose data is corrupt, from pyramid.BaseStackAlgo._read_file: the
    fall-back to the host decoder catches jpeg.read's InvalidOptionError only, so the status word found after the decode
    raises ImageLoadError under "auto" exactly as under "device"."""
    good, bad = stack_files
    fresh = _stacker(jpeg="device", jpeg_split=True)
    try:
        want = fresh.focus_stack(good)
    finally:
        fresh.close()
    assert want.any()
    frames = [jpeg.read(p, "needed") for p in good]
    want_bgr = [jpeg.decode(f) for f in frames]
    out = dev.DeviceBuffer(2 * H * W * 3)
    pusher = jpeg.Pusher(0)
    device, auto = _stacker(jpeg="device", jpeg_split=True), _stacker(jpeg="auto", jpeg_split=True)
    try:
        for path, split, k, status, n in bad:
            frame = jpeg.read(path, split)
            with pytest.raises(ImageLoadError) as e:
                jpeg.decode(frame)
            assert all(t in str(e.value) for t in _names(path, k, n, status)), (path, e.value)
            with pytest.raises(ImageLoadError) as e:
                jpeg.frames_device([good[0], path], out.ptr, split="needed")
            assert all(t in str(e.value) for t in _names(path, k, n, status)), (path, e.value)
            with pytest.raises(ImageLoadError) as e:
                pusher.push(frame, lambda ptr: pytest.fail("a flagged frame was pushed"), lambda: None)
            assert all(t in str(e.value) for t in _names(path, k, n, status)), (path, e.value)
            for stacker in (device, auto):
                with pytest.raises(ImageLoadError) as e:
                    stacker.focus_stack([good[0], path, good[1]])
                assert all(t in str(e.value) for t in _names(path, k, n, status)), (path, e.value)
                assert stacker.skipped == [], stacker.skipped
        # the Pusher that met them decodes good files to the same bytes, the stackers stack them as a fresh one does
        for f, bgr in zip(frames, want_bgr):
            seen = []
            pusher.push(f, lambda ptr: seen.append(pusher.bgr[pusher.k & 1].download(bgr.shape, np.uint8)), lambda: None)
            assert len(seen) == 1
            assert_same(("pusher", f.path), seen[0], bgr)
        for stacker in (device, auto):
            assert_same("stacked", stacker.focus_stack(good), want)
            assert stacker.skipped == []
    finally:
        pusher.close()
        out.free()
        device.close()
        auto.close()
