"""GPU: the site-correction kernels (csrc/kernels_sitecorr.hpp) equal tests/sitecorr_restatement.py bit for bit on the cases of
tests/sitecorr_cases.py -- which test_sitecorr_host.py shows to be meaningful -- in host and device forms; pushes with a
correction set equal the same pushes of the mosaic corrected by hand (the restatement), on the fused output and a level-0 tap;
dng.develop and FocusStack with corrections="auto" equal the same work done by hand; without the option nothing changes.
Every comparison is array_equal."""
import os

import numpy as np
import pytest

import dng_cases as DC
import ljpeg_cases as LC
import sitecorr_cases as SC
import sitecorr_restatement as RS
import unpack_restatement as UR
from shinestacker_amd import Cfa, dng
from shinestacker_amd.demosaic import correct_sites, correct_sites_device, debayer

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


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])


def _device_form(dev, side, name, mosaic, want, run):
    """run(ptr, stream) in place on the mosaic between guard bands: on the null stream, on a handle's stream and (uint16) from a
    buffer that starts 6 bytes off the 16-byte boundary -- other windows, the same samples"""
    out = dev.DeviceBuffer(mosaic.nbytes + 2 * GUARD + 16)
    try:
        for stream, off in ((None, 0), (side.stream, 0)) + (((None, 6),) if mosaic.dtype == np.uint16 else ()):
            raw = np.full(out.nbytes, 0xA5, np.uint8)
            raw[GUARD + off:GUARD + off + mosaic.nbytes] = np.ascontiguousarray(mosaic).view(np.uint8).reshape(-1)
            out.upload(raw)
            run(out.ptr + GUARD + off, stream)
            if stream:
                side.sync()
            else:
                dev.check(dev.load().mi_device_synchronize(0))
            got = out.download((out.nbytes,), np.uint8)
            assert (got[:GUARD + off] == 0xA5).all() and (got[GUARD + off + mosaic.nbytes:] == 0xA5).all(), "the guard band was written"
            assert_same((name, "device", bool(stream), off),
                        got[GUARD + off:GUARD + off + mosaic.nbytes].copy().view(mosaic.dtype).reshape(mosaic.shape), want)
    finally:
        out.free()


@pytest.mark.parametrize("case", SC.CASES, ids=repr)
def test_site_correct_equals_the_restatement(dev, side, case):
    cfa = Cfa(black=list(case.black))
    sc = case.corrections()
    try:
        assert_same((case, "host"), correct_sites(case.mosaic(), cfa, sc), case.expected())
        _device_form(dev, side, case, case.mosaic(), case.expected(),
                     lambda ptr, stream: correct_sites_device(ptr, case.h, case.w, case.dtype, cfa, sc, stream=stream))
    finally:
        sc.close()


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("bad", SC.BAD_CASES + [SC.ONE_PHASE], ids=repr)
def test_bad_sites_equal_the_restatement(dev, side, bad, dtype):
    cfa = Cfa()
    code = dev.DTYPE_CODE[np.dtype(dtype)]
    const = bad.constant(dtype)
    # the constant
    m = bad.mosaic(dtype, True)
    want = RS.repair_const(m, const, bad.mask)
    assert not np.array_equal(want, m)
    sc = dng.SiteCorrections(bad_constant=(const, bad.mask))
    try:
        assert_same((bad, "const host"), correct_sites(m, cfa, sc), want)
        _device_form(dev, side, (bad, "const"), m, want,
                     lambda ptr, stream: correct_sites_device(ptr, bad.h, bad.w, dtype, cfa, sc, stream=stream))
        plane = dev.DeviceBuffer(8 * (-(-bad.h * bad.w // 64)))
        _device_form(dev, side, (bad, "const alone"), m, want, lambda ptr, stream: dev.check(
            dev.load().mi_mosaic_defects_const_device(0, stream, ptr, bad.h, bad.w, code, const, bad.mask, plane.ptr)))
        plane.free()
    finally:
        sc.close()
    # the list
    if bad.mask == 15:
        m = bad.mosaic(dtype, False)
        want = RS.repair_list(m, bad.sites())
        sc = dng.SiteCorrections(bad_sites=bad.sites())
        try:
            assert_same((bad, "list host"), correct_sites(m, cfa, sc), want)
            _device_form(dev, side, (bad, "list"), m, want,
                         lambda ptr, stream: correct_sites_device(ptr, bad.h, bad.w, dtype, cfa, sc, stream=stream))
        finally:
            sc.close()


def test_the_constant_is_judged_on_the_mosaic_as_it_came(dev):
    """a frame where most sites hold the constant, repaired many at once: a repaired neighbour never counts as valid"""
    rng = np.random.default_rng(9)
    m = rng.integers(1, 200, size=(67, 131)).astype(np.uint8)
    m[rng.random(m.shape) < 0.6] = 255
    sc = dng.SiteCorrections(bad_constant=(255, 15))
    want = RS.repair_const(m, 255, 15)
    try:
        for _ in range(2):          # (again: the bit plane of the first call is not what the second one sees)
            assert_same("dense", correct_sites(m, Cfa(), sc), want)
        buf = dev.DeviceBuffer(m.nbytes)
        for _ in range(2):
            buf.upload(m)
            correct_sites_device(buf.ptr, m.shape[0], m.shape[1], m.dtype, Cfa(), sc)
            assert_same("dense, device", buf.download(m.shape, m.dtype), want)
        buf.free()
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------- stacks and files
H, W, N = 21, 37, 3
BLACK = 64                      # in stored 12-bit units


def _file_opcodes():
    nodes = {p: SC.f32(SC._nodes(mv, mh, 30 + p, lo=0.7, hi=1.4)) for p, (mv, mh) in enumerate(((2, 3), (3, 2), (1, 4), (4, 4)))}
    ops = [SC.gain_map_opcode(nodes[p], (p >> 1, p & 1, H, W), pitch=(2, 2)) for p in range(4)]
    ops += [SC.bad_list_opcode(points=[(3, 4), (20, 36)], rects=[(5, 6, 8, 9)]), SC.bad_constant_opcode(4095)]
    dh = [0.25 * (x % 5) - 0.5 for x in range(W)]
    dv = [0.5 - 0.125 * (y % 3) for y in range(H)]
    return ops, {50715: (10, [DC.rational(v) for v in dh]), 50716: (10, [DC.rational(v) for v in dv])}


def _by_hand(frame, mosaic, sc=None):
    """the frame's mosaic corrected by the restatement with the tables of `sc` (default: the file's own)"""
    sc = frame.corrections if sc is None else sc
    q = sc.quantised(mosaic.shape, mosaic.dtype)
    return RS.site_correct(mosaic, frame.cfa.black, q.dh, q.dv, q.gains, q.bad_sites, q.bad_constant)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """three packed and three lossless-JPEG 12-bit DNGs with maps, deltas, a bad list and a constant (some samples hold it);
    the third of each kind carries NO corrections.  (folder, paths, frames, restated mosaics, mosaics corrected by hand)"""
    d = tmp_path_factory.mktemp("sitecorr")
    ops, extra = _file_opcodes()
    out = {}
    for kind in ("packed", "ljpeg"):
        os.makedirs(str(d / kind))
        paths, frames, mosaics, hand = [], [], [], []
        for f in range(N):
            rng = np.random.default_rng([f, 77])
            stored = rng.integers(BLACK + 200, 1500, size=(H, W))
            stored[rng.random((H, W)) < 0.03] = 4095
            p = str(d / kind / f"f{f:02d}.dng")
            own = f != 2
            kw = dict(pattern="GRBG", black=(BLACK,), neutral=(0.55, 1.0, 0.7), matrices={1: (DC.XYZ_D65_MATRIX, 21)})
            if kind == "packed":
                DC.write_dng(p, stored, 12, tile=(16, 16), opcodes2=ops if own else None, extra=extra if own else None, **kw)
            else:
                ex = {**extra, 51009: (7, DC.opcode_list(ops))} if own else None
                LC.write_dng(p, stored, 12, tile=(16, 16), extra=ex, **kw)
            fr = dng.read(p)
            assert (fr.corrections is not None) == own and (not own or fr.corrections.skipped == ())
            m = (stored << 4).astype(np.uint16)
            if kind == "packed":
                assert np.array_equal(UR.unpack_layout(fr.span, fr.layout), m)
            paths.append(p)
            frames.append(fr)
            mosaics.append(m)
            hand.append(_by_hand(fr, m) if own else m)
            assert not own or (hand[-1] != m).mean() > 0.5
        out[kind] = (str(d / kind), paths, frames, mosaics, hand)
    return out


def _stack(dev, mode):
    kw = dict(in_dtype=np.uint16, min_size=8)
    if mode == "float-64":
        kw.update(float_type=dev.MI_F64, arith="exact")
    elif mode == "simple":
        kw.update(impl=dev.IMPL_SIMPLE, arith="exact")
    else:
        kw.update(arith=mode)
    return dev.Stack(H, W, **kw)


def _results(dev, st):
    """a level-0 tap and the fused image"""
    e, i = st.tap(dev.TAP_ENERGY, 0), st.tap(dev.TAP_INDEX, 0)
    return e, i, st.finish()


@pytest.mark.parametrize("mode", ["separable", "exact", "float-64", "simple"])
@pytest.mark.parametrize("kind", ["mosaic", "packed", "ljpeg"])
def test_pushes_with_corrections_equal_pushes_of_the_corrected_mosaic(dev, files, mode, kind):
    """frames 0 and 1 carry corrections, frame 2 none: "auto" clears the setter for it, and only the frames it should are
    affected"""
    _, _, frames, mosaics, hand = files["packed" if kind == "mosaic" else kind]
    develop = frames[0].develop
    with _stack(dev, mode) as st:
        for fr, m in zip(frames, mosaics):
            if kind == "mosaic":
                if fr.corrections is None:
                    st.set_site_correction(None)
                st.push_mosaic(m, fr.cfa, develop=develop, corrections=fr.corrections)
            else:
                st.push_packed(fr, develop=develop, corrections="auto")
        assert kind != "ljpeg" or st.ljpeg_status() == 0
        got = _results(dev, st)
    with _stack(dev, mode) as st:
        for fr, m in zip(frames, hand):
            st.push_mosaic(m, fr.cfa, develop=develop)
        want = _results(dev, st)
    with _stack(dev, mode) as st:
        for fr, m in zip(frames, mosaics):
            st.push_mosaic(m, fr.cfa, develop=develop)
        plain = _results(dev, st)
    for name, g, w, p in zip(("energy", "index", "fused"), got, want, plain):
        assert_same((kind, mode, name), g, w)
    assert not np.array_equal(got[2], plain[2])


def test_the_setter_holds_until_cleared_and_without_it_nothing_changes(dev, files):
    _, _, frames, mosaics, hand = files["packed"]
    sc = frames[0].corrections
    cfa = frames[0].cfa
    # set once: it holds for the pushes behind it, of either kind; cleared: the next frame is untouched; set again
    with _stack(dev, "separable") as st:
        st.set_site_correction(sc)
        st.push_mosaic(mosaics[0], cfa)
        st.push_packed(frames[1])
        st.set_site_correction(None)
        st.push_mosaic(mosaics[1], cfa)
        st.push_mosaic(mosaics[0], cfa, corrections=sc)
        got = _results(dev, st)
    with _stack(dev, "separable") as st:
        for m in (hand[0], _by_hand(frames[1], mosaics[1], sc), mosaics[1], hand[0]):
            st.push_mosaic(m, cfa)
        want = _results(dev, st)
    for g, w in zip(got, want):
        assert_same("setter", g, w)
    # corrections=None, the default: today's outputs bit for bit, on files that carry corrections
    with _stack(dev, "separable") as st:
        for fr in frames:
            st.push_packed(fr, develop=fr.develop)
        got = _results(dev, st)
    with _stack(dev, "separable") as st:
        for fr in frames:
            st.push_packed(fr, develop=fr.develop, corrections=None)
        same = _results(dev, st)
    with _stack(dev, "separable") as st:
        for fr, m in zip(frames, mosaics):
            st.push_mosaic(m, fr.cfa, develop=fr.develop)
        want = _results(dev, st)
    for g, s, w in zip(got, same, want):
        assert_same("default", g, w)
        assert_same("None", s, w)
    # a black level the deltas leave no room for is refused by name, before anything is queued
    with _stack(dev, "separable") as st:
        st.set_site_correction(dng.SiteCorrections(black_h=np.full(W, -5), black_v=np.zeros(H, np.int64)))
        with pytest.raises(ValueError, match="black.* must stay inside"):
            st.push_mosaic(mosaics[0], Cfa(black=3))


@pytest.mark.parametrize("kind", ["packed", "ljpeg"])
def test_unpack_develop_and_frames_device_with_auto(dev, files, kind):
    _, paths, frames, mosaics, hand = files[kind]
    for fr, m, hm in zip(frames, mosaics, hand):
        assert_same("unpack", dng.unpack(fr), m)
        assert_same("unpack auto", dng.unpack(fr, corrections="auto"), hm)
        assert_same("develop", dng.develop(fr), debayer(m, fr.cfa, develop=fr.develop))
        assert_same("develop None", dng.develop(fr, corrections=None), debayer(m, fr.cfa, develop=fr.develop))
        assert_same("develop auto", dng.develop(fr, corrections="auto"), debayer(hm, fr.cfa, develop=fr.develop))
        assert_same("debayer", debayer(m, fr.cfa, corrections=frames[0].corrections), debayer(_by_hand(fr, m, frames[0].corrections), fr.cfa))
    fb = H * W * 3 * 2
    out = dev.DeviceBuffer(N * fb)
    try:
        assert dng.frames_device(paths, out.ptr, corrections="auto") == (H, W, np.dtype(np.uint16))
        for i in range(N):
            assert_same(("frames_device auto", i), out.download((H, W, 3), np.uint16, i * fb), dng.develop(frames[i], corrections="auto"))
        assert dng.frames_device(paths, out.ptr) == (H, W, np.dtype(np.uint16))
        for i in range(N):
            assert_same(("frames_device", i), out.download((H, W, 3), np.uint16, i * fb), dng.develop(frames[i]))
    finally:
        out.free()


def test_focus_stack_on_a_folder_of_dngs_with_auto(dev, files, tmp_path):
    """FocusStack(raw=dng.Raw(corrections="auto")) equals focus_stack_arrays on the mosaics corrected by hand; Raw() equals it
    on the mosaics as they are"""
    import shutil
    from shinestacker_amd import FocusStack, PyramidStack, StackJob
    from shinestacker_amd.imageio import read_img
    _, paths, frames, mosaics, hand = files["packed"]
    work = str(tmp_path)
    os.makedirs(os.path.join(work, "in"))
    for p in paths:
        shutil.copy(p, os.path.join(work, "in"))
    for out, raw, ms in (("out-auto", dng.Raw(corrections="auto"), hand), ("out-plain", dng.Raw(), mosaics)):
        job = StackJob("job", work, input_path="in")
        job.add_action(FocusStack("stack", PyramidStack(min_size=8), input_path="in", output_path=out, raw=raw))
        job.run()
        names = sorted(os.listdir(os.path.join(work, out)))
        assert len(names) == 1, names
        plain = PyramidStack(min_size=8)
        try:
            want = plain.focus_stack_arrays(ms, mosaic=frames[0].cfa, develop=frames[0].develop)
        finally:
            plain.close()
        assert_same(out, read_img(os.path.join(work, out, names[0])), want)
