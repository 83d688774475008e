"""GPU: the split path of the lossless-JPEG decoder (csrc/kernels_ljpeg_split.hpp) on the seeded corrupt DNG files of
tests/dng_mutants.py that dng.read accepts -- the corpus that reached the serial kernel only (test_gpu_dng_mutants.py).

What runs is the raw_ljpeg members of dng_mutants.device_selection(), one and two components, uint8 and uint16 outputs: changed
precisions, predictors and DHT counts, `dht-move`, markers in the middle of a tile, data that ends early, bits that match no
code.  Every segment of every one of them has gone through the plain C++ core on the CPU under sanitizers first
(test_ljpeg_split_core_host.py) and equalled the restatement there.  These are inputs whose complete output the contract
defines ("a corrupt stream costs a status bit and nothing else"); none is chosen to make anything fall over.

    device forms   mi_ljpeg_split_differences_device and mi_raw_ljpeg_split_device between 256-byte guard bands of 0xA5, at 8
                   and 128 bytes a subsequence, with every round, on the null stream and on a handle's stream: the status
                   words and the WHOLE difference plane equal ljpeg_split_restatement.unpack_layout (unreached differences
                   are 0); the unflagged segments of the mosaic equal the serial restatement dng_mutants.restated, segment by
                   segment (tiles share rows); a segment that reports MI_LJPEG_UNDECODED keeps the fill the output was given
    host form      mi_raw_ljpeg_split on the same mutants: the C boundary's checks take what dng.read accepted
    a short span   test_gpu_dng_mutants.py's test, through the split path
    non-vacuity    for every path of ljpeg_split_cases.PATHS, at 8 or at 128 bytes a subsequence, the selection holds a
                   clean-but-changed, a `nocode` and an `overrun` mutant: all fifteen paths are reached (NOT_REACHED is
                   empty).  No accepted mutant carries MI_LJPEG_UNDECODED -- dng.read refuses every descriptor the decoder
                   does not take -- so the check that such a segment keeps its fill stays in place and idle.
    one level up   test_a_flagged_mutant_is_reported_and_the_handle_goes_on with Stack.set_ljpeg_split: ljpeg_status() is the
                   OR of the restated words, and the handle then fuses good frames as a fresh handle does

Everything is array_equal.

Time, measured on the MI355X machine: the `selection` fixture -- the DNG corpus written and parsed, its device selection and
the split restatement of its 162 raw_ljpeg members -- takes 6.6 s, once (21 s on a slower, busier CPU; in one session with
test_gpu_dng_mutants.py the corpus is shared); every test then takes 0.1 to 0.75 s and the whole file 10 s.
"""
import types

import numpy as np
import pytest

import dng_mutants as M
import ljpeg_cases as LC
import ljpeg_split_cases as SC
import ljpeg_split_restatement as S
from shinestacker_amd import dng
from shinestacker_amd.errors import ImageLoadError

pytestmark = pytest.mark.gpu

GUARD = 256         # bytes on either side of the device buffer the kernels write
FILL = 0xA5
ALL_ROUNDS = 0xFFFFFFFF
NOT_REACHED = ()    # the paths of ljpeg_split_cases.PATHS that no selected mutant reaches


def split_selection():
    """[(outcome, the split restatement: mosaic, status words, difference planes)] of the raw_ljpeg members of the device
    selection; host Python only"""
    out = []
    for o in M.device_selection():
        lay = o.frame.layout
        if lay.compression == 7 and lay.spp != 3:
            want = S.unpack_layout(o.frame.span, lay)
            for a in [want[0], want[1]] + want[2]:
                a.setflags(write=False)
            out.append((o, want))
    return out


def flags_of(status):
    return ({"clean"} if not status.any() else set()) | ({"nocode"} if (status & S.NOCODE).any() else set()) | \
        ({"overrun"} if (status & S.OVERRUN).any() else set())


def by_path(selection):
    """{path: the flag classes of the selected mutants that reach it at 8 or at 128 bytes a subsequence}"""
    table = {}
    for o, (_, status, _) in selection:
        segs = S.segments_of(o.frame.span, o.frame.layout)
        for p in set().union(*(SC.paths(None, segs, sub) for sub in SC.SUBS)):
            table.setdefault(p, set()).update(flags_of(status))
    return table


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
    sel = split_selection()
    for o, _ in sel:
        M.restated(o)
    return sel


def test_the_selection_holds_every_class_on_every_path_it_reaches(selection):
    assert len(selection) >= 100
    assert {o.frame.layout.dtype.itemsize for o, _ in selection} == {1, 2}
    assert {int(n) for o, _ in selection for n in o.frame.layout.segments["ncomp"]} == {1, 2}
    table = by_path(selection)
    assert set(table) == set(SC.PATHS) - set(NOT_REACHED), sorted(set(SC.PATHS) - set(table))
    for p, seen in sorted(table.items()):
        assert seen == {"clean", "nocode", "overrun"}, (p, seen)
    assert not any((status & S.UNDECODED).any() for _, (_, status, _) in selection)


def device_form(dev, side, frame, sub, stream, plane, span_bytes=None):
    """(the output between its guard bands, the status words) of the device form with every round: the mosaic, or (`plane`) the
    differences; the output is given FILL everywhere first"""
    lay, L = frame.layout, frame.layout.struct()
    opt = dev.JpegSplitStruct(sub, ALL_ROUNDS)
    up = dng._Staged(frame, 0)
    nspan = up.span_bytes if span_bytes is None else span_bytes
    need = dev.C.c_size_t(0)
    nbytes = len(lay.segments) * lay.seg_height * lay.seg_width * 2 if plane else lay.height * lay.width * lay.dtype.itemsize
    out = scratch = None
    try:
        dev.check(dev.load().mi_ljpeg_split_scratch_bytes(dev.C.byref(L), up.span_bytes, dev.C.byref(opt), dev.C.byref(need)))
        out, scratch = dev.DeviceBuffer(nbytes + 2 * GUARD), dev.DeviceBuffer(need.value)
        out.upload(np.full(out.nbytes, FILL, np.uint8))
        entry = dev.load().mi_ljpeg_split_differences_device if plane else dev.load().mi_raw_ljpeg_split_device
        args = (0, stream, up.buf.ptr, nspan, up.buf.ptr + up.seg_at, dev.C.byref(L)) + (() if plane else (up.table,))
        dev.check(entry(*args, dev.C.byref(opt), scratch.ptr, scratch.nbytes, out.ptr + GUARD, up.status))
        if stream:
            side.sync()
        else:
            dev.check(dev.load().mi_device_synchronize(0))
        raw = out.download((out.nbytes,), np.uint8)
        status = up.buf.download((up.nseg,), np.uint32, up.status_at)
    finally:
        for b in (out, scratch, up.buf):
            if b is not None:
                b.free()
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + nbytes:] == FILL).all(), "the guard band around the output was written"
    return raw[GUARD:GUARD + nbytes].copy(), status


def host_form(dev, frame, sub):
    lay, L = frame.layout, frame.layout.struct()
    got = np.full((lay.height, lay.width), FILL * 0x0101 & np.iinfo(lay.dtype).max, lay.dtype)
    st = np.full(len(lay.segments), 0xFFFFFFFF, np.uint32)
    span = dng.host_span(frame)
    table = None if lay.table is None else lay.table.ctypes.data
    opt = dev.JpegSplitStruct(sub, 0)
    dev.check(dev.load().mi_raw_ljpeg_split(0, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, dev.C.byref(L), table, dev.C.byref(opt),
                                            got.ctypes.data, st.ctypes.data))
    return got, st


def check_mosaic(name, lay, got, st, status, serial):
    """the status words are the restatement's; an unflagged segment equals the serial restatement's, an UNDECODED one keeps
    the fill.  Segment by segment: tiles share rows."""
    assert st.tolist() == status.tolist(), (name, st.tolist(), status.tolist())
    nsx = lay.grid[1]
    fill = np.asarray(FILL * 0x0101 & np.iinfo(lay.dtype).max, lay.dtype)
    for k in range(len(status)):
        y0, x0 = (k // nsx) * lay.seg_height - lay.crop_y, (k % nsx) * lay.seg_width - lay.crop_x
        ys, xs = slice(max(y0, 0), max(y0 + lay.seg_height, 0)), slice(max(x0, 0), max(x0 + lay.seg_width, 0))
        if status[k] == 0:
            assert np.array_equal(got[ys, xs], serial[ys, xs]), (name, k, int((got[ys, xs] != serial[ys, xs]).sum()))
        elif status[k] & S.UNDECODED:
            assert (got[ys, xs] == fill).all(), (name, k)


def check_planes(name, lay, raw, st, status, planes):
    assert st.tolist() == status.tolist(), (name, st.tolist(), status.tolist())
    got = raw.view(np.uint16).reshape(len(planes), lay.seg_height, lay.seg_width)
    for k, want in enumerate(planes):
        assert np.array_equal(got[k, :want.shape[0]], want), (name, k, int((got[k, :want.shape[0]] != want).sum()))
        assert not got[k, want.shape[0]:].any(), (name, k)


@pytest.mark.parametrize("stream", ["null-stream", "side-stream"])
@pytest.mark.parametrize("sub", SC.SUBS)
def test_the_device_forms_equal_the_restatements_on_the_mutants(dev, side, selection, sub, stream):
    for o, (_, status, planes) in selection:
        lay, s = o.frame.layout, side.stream if stream == "side-stream" else None
        raw, st = device_form(dev, side, o.frame, sub, s, plane=True)
        check_planes((o.recipe, sub), lay, raw, st, status, planes)
        raw, st = device_form(dev, side, o.frame, sub, s, plane=False)
        check_mosaic((o.recipe, sub), lay, raw.view(lay.dtype).reshape(lay.height, lay.width), st, status, M.restated(o)[0])


@pytest.mark.parametrize("sub", SC.SUBS)
def test_the_host_form_equals_the_restatements_on_the_mutants(dev, selection, sub):
    for o, (_, status, _) in selection:
        got, st = host_form(dev, o.frame, sub)
        check_mosaic((o.recipe, sub), o.frame.layout, got, st, status, M.restated(o)[0])


def test_a_span_declared_short_reads_nothing_beyond_it(dev, side):
    """every one- and two-component base of several compressed segments (the heavy ones aside) with its span DECLARED shorter
    than the buffer that holds it, at three seeded cut points: bytes at or beyond span_bytes count as absent, as the
    restatement cuts the data there"""
    ran = 0
    for b in M.bases():
        frame = M.base_outcome(b).frame
        lay = frame.layout
        if b.reader != "raw_ljpeg" or b.heavy or not b.restate or len(lay.segments) < 2:
            continue
        rng = np.random.default_rng([b.index, 113])
        first = int(lay.segments["scan_off"].min())
        for i, short in enumerate(sorted(int(v) for v in rng.integers(first + 1, frame.span.nbytes, size=3))):
            cut = types.SimpleNamespace(layout=lay, span=frame.span[:short])
            _, status, planes = S.unpack_layout(cut.span, lay)
            assert status.any(), (b, short)
            sub = SC.SUBS[i & 1]
            raw, st = device_form(dev, side, frame, sub, None, plane=True, span_bytes=short)
            check_planes((b, short), lay, raw, st, status, planes)
            raw, st = device_form(dev, side, frame, sub, side.stream, plane=False, span_bytes=short)
            check_mosaic((b, short), lay, raw.view(lay.dtype).reshape(lay.height, lay.width), st, status, M.restate(cut)[0])
            ran += 1
    assert ran >= 45


# ---------------------------------------------------------------------------------------------- one level up
H, W = 72, 104


def _stored(f):
    """a smooth 12-bit mosaic with a little noise over a black level of 256"""
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng([H, W, f, 127])
    return np.clip(256 + 20 * xx + 11 * yy + 300 * f + rng.integers(-9, 10, size=(H, W)), 0, 4095).astype(np.int64)


@pytest.fixture(scope="module")
def stack_frames(tmp_path_factory):
    """(two good frames in strips of 7 rows; ten mutants of the first whose split restatement's status is not 0, with it)"""
    d = tmp_path_factory.mktemp("mutant-stack")
    good, infos = [], []
    for f in range(2):
        p = str(d / f"f{f}.dng")
        infos.append(LC.write_dng(p, _stored(f), 12, ncomp=2, rows_per_strip=7, pattern="GRBG", black=(256,)))
        good.append(dng.read(p))
    with open(str(d / "f0.dng"), "rb") as fh:
        b = M.Base("stack/f0", "raw_ljpeg", fh.read(), infos[0], samples=H * W)
    b.index = len(M.bases())
    bad, early = [], 0
    for m in M.jpeg_mutants(b):
        if len(bad) == 10:
            break
        if not m.kind.startswith(("scan-", "dht-move")):
            continue
        o = M.parse(b, m)
        if o.accepted and o.frame.layout.compression == 7:
            status = S.unpack_layout(o.frame.span, o.frame.layout)[1]
            only_early = not (status & S.NOCODE).any()
            if status.any() and (not only_early or early < 6):      # (data that ends early is the common one: six at the most)
                early += only_early
                bad.append((o, status))
    assert len(bad) == 10 and early == 6
    return good, bad


def test_a_flagged_mutant_is_reported_and_the_handle_goes_on(dev, stack_frames):
    good, bad = stack_frames
    kw = dict(in_dtype=np.uint16, min_size=16, arith="separable")
    with dev.Stack(H, W, **kw) as st:
        for fr in good:
            st.push_packed(fr)
        assert st.ljpeg_status() == 0
        want = st.finish()
    assert want.any()
    with dev.Stack(H, W, **kw) as st:
        st.set_ljpeg_split(True)
        for i, (o, status) in enumerate(bad):
            k = int(np.flatnonzero(status)[0])
            with pytest.raises(ImageLoadError) as e:
                dng.unpack(o.frame, split=True)
            assert o.frame.path in str(e.value) and f"segment {k} " in str(e.value) and f"status {int(status[k])}:" in str(e.value), (o.recipe, e.value)
            if i & 1:
                st.set_ljpeg_split({"sub_bytes": 8})
            st.push_packed(o.frame)
            assert st.ljpeg_status() == int(np.bitwise_or.reduce(status)), o.recipe
            assert st.ljpeg_status() == 0, o.recipe         # (cleared by the read)
        st.reset()
        for fr in good:
            st.push_packed(fr)
        assert st.ljpeg_status() == 0
        got = st.finish()
    assert np.array_equal(got, want)
