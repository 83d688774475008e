"""GPU: the split path of the lossless-JPEG decoder (csrc/kernels_ljpeg_split.hpp) equals its restatement
(tests/ljpeg_split_restatement.py) bit for bit on the cases of tests/ljpeg_split_cases.py -- the difference plane and the
status words at 8 and 128 bytes a subsequence -- and its samples equal the writer's own and the serial kernel's (mi_raw_ljpeg)
in host form and in device form; with one round where the never-synchronising segment needs two the device form says so for
that segment alone and the host form repairs it; and the layers above (dng.unpack(split=), Stack.set_ljpeg_split,
FocusStack(raw=Raw(ljpeg_split=True))) equal the same call without the option.  Every comparison is array_equal; corrupt
streams come from the short cases and the seeded mutants only, and end with status bits."""
import os

import numpy as np
import pytest

import dng_cases as DC
import ljpeg_cases as LC
import ljpeg_split_cases as SC
import ljpeg_split_restatement as S
from shinestacker_amd import dng

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]       # (every test's GPU steps under one time limit of its own)

GUARD = 256         # bytes on either side of the device buffer the kernels write
SHORT = {c.name: (k, flag) for c, k, flag in SC.SHORT}


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
def table(dev, tmp_path_factory):
    """{case name: (DngFrame, the restated mosaic, status words and difference planes, the serial kernel's mosaic and status)}:
    written, parsed, restated and decoded by mi_raw_ljpeg once"""
    d = tmp_path_factory.mktemp("ljpeg_split")
    out = {}
    for c in SC.ALL:
        c.write(str(d / (c.name + ".dng")))
        frame = dng.read(str(d / (c.name + ".dng")))
        want, status, planes = S.unpack_layout(frame.span, frame.layout)
        serial, sstatus = _host(dev, frame, None)
        for a in [want, status, serial, sstatus] + planes:
            a.setflags(write=False)
        out[c.name] = (frame, want, status, planes, serial, sstatus)
    return out


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def _opt(dev, sub=0, rounds=0):
    return dev.JpegSplitStruct(sub, rounds)


def _host(dev, frame, opt):
    """(mosaic, status) of the host form: mi_raw_ljpeg (opt None) or mi_raw_ljpeg_split"""
    lay, L = frame.layout, frame.layout.struct()
    got = np.zeros((lay.height, lay.width), lay.dtype)
    st = np.full(len(lay.segments), 0xFFFFFFFF, np.uint32)
    span = dng.host_span(frame)
    table = None if lay.table is None else lay.table.ctypes.data
    if opt is None:
        dev.check(dev.load().mi_raw_ljpeg(0, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, dev.C.byref(L), table, got.ctypes.data,
                                          st.ctypes.data))
    else:
        dev.check(dev.load().mi_raw_ljpeg_split(0, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, dev.C.byref(L), table,
                                                dev.C.byref(opt), got.ctypes.data, st.ctypes.data))
    return got, st


def _device(dev, side, frame, opt, stream, plane=False):
    """(the output between its guard bands, the status words) of the device form: the mosaic, or (`plane`) the differences"""
    lay, L = frame.layout, frame.layout.struct()
    up = dng._Staged(frame, 0)
    need = dev.C.c_size_t(0)
    dev.check(dev.load().mi_ljpeg_split_scratch_bytes(dev.C.byref(L), up.span_bytes, dev.C.byref(opt), dev.C.byref(need)))
    nbytes = len(lay.segments) * lay.seg_height * lay.seg_width * 2 if plane else lay.height * lay.width * lay.dtype.itemsize
    out, scratch = dev.DeviceBuffer(nbytes + 2 * GUARD), dev.DeviceBuffer(need.value)
    try:
        out.upload(np.full(out.nbytes, 0xA5, np.uint8))
        if plane:
            dev.check(dev.load().mi_ljpeg_split_differences_device(0, stream, up.buf.ptr, up.span_bytes, up.buf.ptr + up.seg_at, dev.C.byref(L),
                                                                   dev.C.byref(opt), scratch.ptr, scratch.nbytes, out.ptr + GUARD, up.status))
        else:
            dev.check(dev.load().mi_raw_ljpeg_split_device(0, stream, up.buf.ptr, up.span_bytes, up.buf.ptr + up.seg_at, dev.C.byref(L), up.table,
                                                           dev.C.byref(opt), scratch.ptr, scratch.nbytes, out.ptr + GUARD, up.status))
        if stream:
            side.sync()
        else:
            dev.check(dev.load().mi_device_synchronize(0))
        raw = out.download((out.nbytes,), np.uint8)
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + nbytes:] == 0xA5).all(), "the guard band around the output was written"
        return raw[GUARD:GUARD + nbytes].copy(), up.buf.download((up.nseg,), np.uint32, up.status_at)
    finally:
        out.free()
        scratch.free()
        up.buf.free()


def _keep(case, lay, status):
    """the output rows whose segments are unflagged (the short cases are strips)"""
    keep = np.ones(lay.height, bool)
    for k in np.flatnonzero(status):
        keep[k * lay.seg_height:(k + 1) * lay.seg_height] = False
    return keep


@pytest.mark.parametrize("sub", SC.SUBS)
@pytest.mark.parametrize("case", SC.ALL, ids=repr)
def test_the_difference_plane_and_status_equal_the_restatement(dev, side, table, case, sub):
    """the host form (exact rounds), and the device form with every round on a handle's stream"""
    frame, _, status, planes, _, _ = table[case.name]
    lay, L = frame.layout, frame.layout.struct()
    shape = (len(lay.segments), lay.seg_height, lay.seg_width)
    span = dng.host_span(frame)
    got = np.full(shape, 0xA5A5, np.uint16)
    st = np.full(shape[0], 0xFFFFFFFF, np.uint32)
    opt = _opt(dev, sub)
    dev.check(dev.load().mi_ljpeg_split_differences(0, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, dev.C.byref(L), dev.C.byref(opt),
                                                    got.ctypes.data, st.ctypes.data))
    raw, dst = _device(dev, side, frame, _opt(dev, sub, 0xFFFFFFFF), side.stream, plane=True)
    for name, g, s in (("host", got, st), ("device", raw.view(np.uint16).reshape(shape), dst)):
        assert s.tolist() == status.tolist(), (case, name)
        for k, want in enumerate(planes):
            assert_same((case, name, k), g[k, :want.shape[0]], want)
            assert not g[k, want.shape[0]:].any(), (case, name, k)


@pytest.mark.parametrize("case", SC.ALL, ids=repr)
def test_the_split_path_equals_the_stored_samples_and_the_serial_kernel(dev, side, table, case):
    """host form at the default and at 8 bytes a subsequence; device form on the null stream and on a handle's stream"""
    frame, want, status, _, serial, sstatus = table[case.name]
    lay = frame.layout
    if case.name in SHORT:
        k, flag = SHORT[case.name]
        assert status[k] & flag and not np.delete(status, k).any() and status.tolist() == sstatus.tolist()
    else:
        assert not status.any() and not sstatus.any()
        assert_same((case, "the restatement"), want, serial)
        if case in SC.WHOLE:
            assert_same((case, "the writer"), want, case.expected())
    keep = _keep(case, lay, status)
    for sub in (0, 8):
        got, st = _host(dev, frame, _opt(dev, sub))
        assert st.tolist() == status.tolist(), (case, sub)
        assert_same((case, "host", sub), got[keep], serial[keep])
    for stream, sub in ((None, 0), (side.stream, 8)):
        raw, st = _device(dev, side, frame, _opt(dev, sub, 0xFFFFFFFF), stream)
        assert st.tolist() == status.tolist(), (case, stream)
        assert_same((case, "device", stream), raw.view(lay.dtype).reshape(serial.shape)[keep], serial[keep])


def test_seeded_mutants_end_with_status_bits(dev, table):
    """corrupt data costs status bits and nothing else: the status words are the restatement's, unflagged segments the serial
    kernel's"""
    rng = np.random.default_rng(2028)
    flagged = 0
    for name in SC.MUTATED:
        frame = table[name][0]
        lay = frame.layout
        for m in SC.mutants(bytes(frame.span), lay, rng, n=4):
            span = np.frombuffer(m, np.uint8)
            bad = dng.DngFrame(frame.path, lay, span, frame.cfa, frame.develop, None, 1, ())
            _, status, _ = S.unpack_layout(span, lay)
            serial, sstatus = _host(dev, bad, None)
            got, st = _host(dev, bad, _opt(dev, 8))
            assert (st != 0).tolist() == (status != 0).tolist() == (sstatus != 0).tolist(), name
            assert st.tolist() == status.tolist(), name
            nsx = lay.grid[1]
            for k in np.flatnonzero(status == 0):       # segment by segment: tiles share rows
                y0, x0 = (k // nsx) * lay.seg_height - lay.crop_y, (k % nsx) * lay.seg_width - lay.crop_x
                ys, xs = slice(max(y0, 0), max(y0 + lay.seg_height, 0)), slice(max(x0, 0), max(x0 + lay.seg_width, 0))
                assert_same((name, int(k)), got[ys, xs], serial[ys, xs])
            flagged += int((status != 0).sum())
    assert flagged > 5


def test_one_round_leaves_the_never_synchronising_segment_unsynced_and_says_so(dev, side, table):
    """sub_bytes 8, max_rounds 1: the first strip needs two rounds and reports MI_LJPEG_UNSYNCED, that bit alone; the ordinary
    strip beside it in the same span is exact.  The host form, given the same option, runs again and returns every sample."""
    frame, want, status, _, serial, _ = table[SC.NEVER_BESIDE.name]
    lay = frame.layout
    assert not status.any() and lay.seg_height == 24 and len(lay.segments) == 2
    assert_same("the restatement", want, serial)
    for stream in (None, side.stream):
        raw, st = _device(dev, side, frame, _opt(dev, 8, 1), stream)
        assert st.tolist() == [dev.LJPEG_UNSYNCED, 0]
        assert_same("the ordinary strip", raw.view(lay.dtype).reshape(want.shape)[24:], want[24:])
    raw, st = _device(dev, side, frame, _opt(dev, 8, 2), None)
    assert st.tolist() == [0, 0]
    assert_same("two rounds", raw.view(lay.dtype).reshape(want.shape), want)
    got, st = _host(dev, frame, _opt(dev, 8, 1))
    assert st.tolist() == [0, 0]
    assert_same("host", got, want)


def test_unpack_with_split_equals_unpack(dev, table):
    for c in SC.WHOLE:
        frame = table[c.name][0]
        plain = dng.unpack(frame)
        assert_same(c, dng.unpack(frame, split=True), plain)
        assert_same(c, plain, c.expected())
    assert_same("options", dng.unpack(table[SC.NEVER.name][0], split={"sub_bytes": 8, "max_rounds": 1}), SC.NEVER.expected())
    from shinestacker_amd.errors import ImageLoadError
    with pytest.raises(ImageLoadError, match="segment 1"):
        dng.unpack(table["short-cut-mid-data"][0], split=True)


def test_with_the_option_off_nothing_changes(dev, side, table):
    """the serial entry point's output, as the table took it before any split call, is what it returns now"""
    for name in ("12bit-tiles-21x37-shuffled", "16bit-64x130-random-long-stream", "short-marker-mid-data"):
        frame, _, _, _, serial, sstatus = table[name]
        got, st = _host(dev, frame, None)
        assert st.tolist() == sstatus.tolist()
        assert_same(name, got, serial)


# ---------------------------------------------------------------------------------------------- stacks
H, W = 72, 308      # (a never-synchronising frame of this shape: 11 088 pixels of three zero bits, 4158 bytes, three groups at 8)
COLOUR = dict(pattern="GRBG", black=(256,), neutral=(0.55, 1.0, 0.7), matrices={1: (DC.XYZ_D65_MATRIX, 21)})


@pytest.fixture(scope="module")
def stack_files(tmp_path_factory):
    """frames of one shape: the never-synchronising one, two of noise on a ramp as tiles and as strips with predictor 6, and one
    uncompressed; (the parsed frames, their mosaics)"""
    d = tmp_path_factory.mktemp("stack")
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = [np.clip(600 + 3 * xx + 40 * yy + rng.integers(-30, 31, size=(H, W)), 0, 4095).astype(np.int64) for _ in range(3)]
    never = np.full((H, W), 2048, np.int64)
    paths = [str(d / f"f{i}.dng") for i in range(4)]
    LC.write_dng(paths[0], never, 12, ncomp=2, tables=[SC.ONE_BIT, SC.TWO_BITS], **COLOUR)
    LC.write_dng(paths[1], ramp[0], 12, ncomp=2, tile=(32, 128), odd_start=True, **COLOUR)
    LC.write_dng(paths[2], ramp[1], 12, ncomp=1, predictor=6, rows_per_strip=7, **COLOUR)
    DC.write_dng(paths[3], ramp[2], 12, rows_per_strip=7, **COLOUR)
    frames = [dng.read(p) for p in paths]
    assert S.groups_touched(S.segments_of(frames[0].span, frames[0].layout), 8) == 3
    return paths, frames, [(m << 4).astype(np.uint16) for m in (never, ramp[0], ramp[1], ramp[2])]


@pytest.mark.parametrize("mode", ["separable", "float-64"])
def test_pushes_with_the_split_path_equal_pushes_without(dev, stack_files, mode):
    """compressed frames -- the never-synchronising one among them, at 8 bytes a subsequence so that it needs its rounds --
    beside a packed and a mosaic push on one handle, asynchronous and synchronous route: fused output and status word"""
    _, frames, mosaics = stack_files
    kw = dict(in_dtype=np.uint16, min_size=16)
    kw.update(dict(float_type=dev.MI_F64, arith="exact") if mode == "float-64" else dict(arith=mode))
    cfa, develop = frames[1].cfa, frames[1].develop
    outs = []
    for split in (False, {"sub_bytes": 8}, True):
        with dev.Stack(H, W, **kw) as st:
            if split:
                st.set_ljpeg_split(split)
            st.push_packed(frames[0], develop=develop)
            st.push_packed(frames[1], develop=develop)
            st.push_packed(frames[3], develop=develop)
            st.push_mosaic(mosaics[2], cfa, develop=develop)
            st.push_packed(frames[2], develop=develop)
            if split:
                st.set_ljpeg_split(False)       # cleared: the serial kernel again, on the same handle
            st.push_packed(frames[1], develop=develop)
            assert st.ljpeg_status() == 0
            outs.append(st.finish())
    with dev.Stack(H, W, **kw) as st:
        for m in (mosaics[0], mosaics[1], mosaics[3], mosaics[2], mosaics[2], mosaics[1]):
            st.push_mosaic(m, cfa, develop=develop)
        want = st.finish()
    for got in outs:
        assert_same(mode, got, want)
    assert want.any()


def test_a_short_stream_still_raises_the_status_word(dev, stack_files, tmp_path):
    _, frames, _ = stack_files
    p = str(tmp_path / "bad.dng")
    rng = np.random.default_rng(6)
    LC.write_dng(p, rng.integers(0, 4096, size=(H, W)), 12, ncomp=2, rows_per_strip=7, mangle=LC._cut, **COLOUR)
    bad = dng.read(p)
    with dev.Stack(H, W, in_dtype=np.uint16, min_size=16, arith="separable") as st:
        st.set_ljpeg_split(True)
        st.push_packed(frames[1])
        assert st.ljpeg_status() == 0
        st.push_packed(bad)
        assert st.ljpeg_status() == S.OVERRUN and st.ljpeg_status() == 0
    with pytest.raises(ValueError):
        dev.ljpeg_split_options({"rounds": 3})


def test_develop_frames_device_and_focus_stack_take_the_option(dev, stack_files, tmp_path):
    import shutil
    from shinestacker_amd import FocusStack, PyramidStack, StackJob
    from shinestacker_amd.imageio import read_img
    paths, frames, _ = stack_files
    for f in frames[:3]:
        assert_same(f.path, dng.develop(f, split=True), dng.develop(f))
    fb = H * W * 3 * 2
    a, b = dev.DeviceBuffer(3 * fb), dev.DeviceBuffer(3 * fb)
    try:
        assert dng.frames_device(paths[:3], a.ptr, split={"sub_bytes": 8}) == dng.frames_device(paths[:3], b.ptr) == (H, W, np.dtype(np.uint16))
        assert_same("frames_device", a.download((3, H, W, 3), np.uint16), b.download((3, H, W, 3), np.uint16))
    finally:
        a.free()
        b.free()
    work = str(tmp_path)
    os.makedirs(os.path.join(work, "in"))
    for p in paths:
        shutil.copy(p, os.path.join(work, "in"))
    job = StackJob("job", work, input_path="in")
    job.add_action(FocusStack("plain", PyramidStack(min_size=16), input_path="in", output_path="out-plain", raw=dng.Raw()))
    job.add_action(FocusStack("split", PyramidStack(min_size=16), input_path="in", output_path="out-split", raw=dng.Raw(ljpeg_split=True)))
    job.run()
    names = sorted(os.listdir(os.path.join(work, "out-plain")))
    assert len(names) == 1 and sorted(os.listdir(os.path.join(work, "out-split"))) == names
    assert_same("FocusStack", read_img(os.path.join(work, "out-split", names[0])), read_img(os.path.join(work, "out-plain", names[0])))
