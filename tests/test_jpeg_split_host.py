"""CPU: the split JPEG decoder's definition (tests/jpeg_split_restatement.py) and the reader's `split=` option.

  * walk_split equals jpeg_restatement.walk, planes and status words, on every clean case of tests/jpeg_split_cases.py and
    on every case of tests/jpeg_cases.py: where a stream is whole the two walks take the same symbols;
  * on the short streams it raises the bit each is there for (it differs from the serial walker in what it leaves in blocks it
    does not reach: zeros, not what zero bits decode to);
  * where PIL imports: Pillow's own default files -- no restart markers; every size, subsampling and quality of
    jpeg_cases.pillow_files' grid -- decode through walk_split array_equal to Pillow;
  * no case is vacuous: the table holds every feature it names, the scan that starts a subsequence on a stuffed 00 does, and
    the dense pictures need more than one round across groups of 256 subsequences of 8 bytes;
  * a lane's entry never lies beyond its own subsequence: a symbol reaches at most 8 bytes of the span, so the pass-through
    the scheme provides for is never taken at sub_bytes >= 8 (the stream of FF 00 pairs is the case that was to take it);
  * jpeg.read(split=...) agrees with the lenient parser, marks the frames as stated, and keeps every other refusal."""
import io

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_restatement as R
import jpeg_split_cases as SC
import jpeg_split_restatement as S

CLEAN = SC.PLAIN + SC.LONG + SC.ALWAYS


def _same(name, a, b):
    (pa, sa), (pb, sb) = a, b
    assert np.array_equal(sa, sb), (name, sa, sb)
    assert len(pa) == len(pb)
    for x, y in zip(pa, pb):
        assert x.dtype == y.dtype and np.array_equal(x, y), name


def test_walk_split_equals_the_serial_walk_on_clean_streams():
    names = [c.name for c in SC.PLAIN] + [c.name for c in SC.LONG]
    assert len(set(names)) == len(names)
    for c in CLEAN + JC.CASES:
        h = R.parse(c.data())
        want = R.walk(c.data(), h, dri=h["dri"] or _mcus(h))
        assert not want[1].any(), c
        _same(c.name, S.walk_split(c.data(), h), want)


def _mcus(h):
    _, mx, my = R.geometry(h)
    return mx * my


def test_short_streams_raise_their_bits():
    alone = set()
    for c, bit in SC.SHORT:
        h = R.parse(c.data())
        assert len(h["offsets"]) == 2, c
        planes, status = S.walk_split(c.data(), h)
        assert int(status[0]) & bit, (c, status)
        if int(status[0]) == bit:
            alone.add(bit)
    assert alone == {S.NOCODE, S.OVERRUN, S.RUN}
    # what is not reached stays 0, and its DC is its predecessor's: the truncated picture, block by block
    c = next(c for c, _ in SC.SHORT if c.name == "short-truncated")
    h = R.parse(c.data())
    planes, status = S.walk_split(c.data(), h)
    whole = R.walk(JC.write(**{**c.kw, "tweak": None}), h, dri=_mcus(h))[0]
    assert status.tolist() == [S.OVERRUN]
    assert np.array_equal(planes[0][0], whole[0][0]) and not np.array_equal(planes[0], whole[0])
    last = planes[0][-1, -1]
    assert not last[1:].any() and last[0] == planes[0][-1, -2][0]


def _pillow(data):
    from PIL import Image
    a = np.array(Image.open(io.BytesIO(data)))
    return np.repeat(a[:, :, None], 3, 2) if a.ndim == 2 else np.ascontiguousarray(a[:, :, ::-1])


def pillow_plain_files():
    """pillow_files' pictures, sizes, subsamplings and qualities as Pillow writes them by default: no restart markers"""
    from PIL import Image
    out = []
    for (h, w) in JC.SIZES:
        rgb = JC.picture(h, w, h + w)
        for sub, mode in ((0, "444"), (1, "422"), (2, "420"), (None, "grey")):
            for q in (30, 90, 100):
                for kw in ({}, {"optimize": True}):
                    b = io.BytesIO()
                    Image.fromarray(rgb if sub is not None else rgb[:, :, 1]).save(b, "JPEG", quality=q, **({} if sub is None else {"subsampling": sub}), **kw)
                    out.append((f"pil-{h}x{w}-{mode}-q{q}-{'-'.join(kw) or 'default'}", b.getvalue()))
    for (h, w) in JC.NARROW:
        rgb = JC.picture(h, w, 7 * h + w)
        for sub, mode in ((1, "422"), (2, "420")):
            b = io.BytesIO()
            Image.fromarray(rgb).save(b, "JPEG", quality=95, subsampling=sub)
            out.append((f"pil-narrow-{h}x{w}-{mode}", b.getvalue()))
    return out


def test_the_restatement_equals_pillow_on_pillow_s_default_files():
    pytest.importorskip("PIL")
    files = pillow_plain_files()
    assert len(files) == 6 * 4 * 3 * 2 + 2 * len(JC.NARROW)
    for name, data in files:
        h = R.parse(data)
        assert h["dri"] == 0 and len(h["offsets"]) == 2, name
        planes, status = S.walk_split(data, h)
        assert not status.any() and np.array_equal(R.render(planes, h), _pillow(data)), name


def test_the_writer_s_plain_cases_equal_pillow():
    pytest.importorskip("PIL")
    compared = 0
    for c in SC.PLAIN:
        if c.codec:
            h = R.parse(c.data())
            planes, status = S.walk_split(c.data(), h)
            assert not status.any() and np.array_equal(R.render(planes, h), _pillow(c.data())), c
            compared += 1
    assert compared >= len(SC.PLAIN) - 2


def test_no_case_is_vacuous():
    by_name = {c.name: c for c in SC.PLAIN}
    seen = set()
    for name, feature in (("full-block", "noeob"), ("zrl-runs", "zrl"), ("len16-code", "len16"), ("category-15", "cat15"),
                          ("dc-category-15", "dc-cat15"), ("ff-first", "ff-first"), ("ff-middle", "ff-middle"), ("ff-last", "ff-last")):
        data = by_name[name].data()
        h = R.parse(data)
        assert h["dri"] == 0 and len(h["offsets"]) == 2
        trace = set()
        R.walk(data, h, dri=_mcus(h), trace=trace)
        assert feature in trace, (name, trace)
        seen |= trace
    assert SC.FEATURES <= seen
    for (hh, ww) in JC.SIZES:
        for mode in JC.MODES:
            assert f"{hh}x{ww}-{mode}" in by_name
    for (hh, ww) in JC.NARROW:
        assert f"narrow-{hh}x{ww}-422" in by_name and f"narrow-{hh}x{ww}-420" in by_name
    # a subsequence of 8 bytes that begins on the 00 of an FF 00 pair, and its cold state one byte later
    data = by_name["stuffed-00-first"].data()
    h = R.parse(data)
    starts = SC.stuffed_starts(SC.scan_of(data), 8)
    assert starts
    iv = S.Interval(data[h["offsets"][0]:h["offsets"][1]])
    assert S.cold(iv, 8 * starts[0]) == (8 * starts[0] + 1, 0, 0, 0) and S.cold(iv, 8) in ((8, 0, 0, 0), (9, 0, 0, 0))
    # DRI above the serial walker's limit, and files with intervals for "always", one of them with more than 64
    assert all(R.parse(c.data())["dri"] == 8193 for c in SC.LONG)
    assert {c.name for c in SC.ALWAYS} >= {"37x53-444-dri1", "37x53-444-dri3", "37x53-420-dri1", "129x150-420-dri1"}
    # the slow convergence: more than one round across groups, none at 128 bytes
    for name in SC.SLOW:
        data = by_name[name].data()
        h = R.parse(data)
        assert S.rounds_needed(data, h, 8, 256) > 1, name
        assert S.rounds_needed(data, h, 128, 256) <= 1, name
    assert S.rounds_needed(by_name["37x53-444"].data(), R.parse(by_name["37x53-444"].data()), 8, 256) >= 0


def test_the_cold_exits_join_the_true_ones_and_no_entry_skips_a_lane():
    """the exits from the cold states differ from the true ones somewhere (else the fix point would be idle) and agree
    somewhere behind; and a true entry lies in the lane's own subsequence, at the latest in its last byte"""
    by_name = {c.name: c for c in SC.PLAIN}
    farthest = 0
    for name, sub in (("129x150-420-fine", 8), ("37x53-420", 16), ("129x150-444-fine", 128)):
        data = by_name[name].data()
        h = R.parse(data)
        ex = S.exits(data, h, sub)
        differ = [c[0] != t[0] for c, t in ex]
        assert any(differ[1:]) and not differ[0], name
        if sub == 8:
            assert not all(differ[1:]), name
    c = next(c for c, _ in SC.SHORT if c.name == "ff00-pairs")
    for data in [c.data()] + [by_name[n].data() for n in ("129x150-444-fine", "stuffed-00-first")]:
        h = R.parse(data)
        prev = None
        for (iv, lo, hi, last), (_, (t, _)) in zip(S.lanes_of(data, h, 8), S.exits(data, h, 8)):
            if prev is not None and prev is not S.END and not last:
                assert lo <= prev[0] < hi
                farthest = max(farthest, prev[0] - lo)
            prev = t
    assert 0 < farthest <= 7


@pytest.fixture(scope="module")
def jpeg():
    from shinestacker_amd import jpeg
    return jpeg


def test_read_split_agrees_with_the_lenient_parser(jpeg, tmp_path):
    from shinestacker_amd.errors import InvalidOptionError
    for case in SC.PLAIN + SC.LONG + [s[0] for s in SC.SHORT]:
        path = case.write(str(tmp_path / "case.jpg"))
        h = R.parse(case.data())
        with pytest.raises(InvalidOptionError, match="DRI = "):
            jpeg.read(path)
        for mode in ("needed", "always"):
            f = jpeg.read(path, split=mode)
            assert f.split is True and f.split_options == (0, 0)
            assert f.shape == (h["height"], h["width"]) and f.ncomp == h["ncomp"] and f.sampling == (h["hmax"], h["vmax"]), case
            assert f.dri == h["dri"] and f.n_intervals == 1 and f.desc.n_intervals == 1 and f.desc.dri == _mcus(h), case
            assert (f.offsets.astype(int) + h["scan_off"]).tolist() == h["offsets"], case
            assert bytes(f.span[:h["offsets"][-1] - h["scan_off"]]) == case.data()[h["scan_off"]:h["offsets"][-1]]
    for case in SC.ALWAYS:
        path = case.write(str(tmp_path / "case.jpg"))
        h = R.parse(case.data())
        a, b, c = jpeg.read(path), jpeg.read(path, split="needed"), jpeg.read(path, split="always")
        assert (a.split, b.split, c.split) == (False, False, True)
        for f in (a, b, c):
            assert f.dri == h["dri"] == f.desc.dri and f.n_intervals == len(h["offsets"]) - 1
            assert (f.offsets.astype(int) + h["scan_off"]).tolist() == h["offsets"]
    with pytest.raises(InvalidOptionError, match="split = maybe"):
        jpeg.read(path, split="maybe")


def test_every_other_refusal_stands_under_split(jpeg, tmp_path):
    from shinestacker_amd.errors import InvalidOptionError
    lifted = {"no-restart-interval", "restart-interval-too-long"}
    assert lifted <= {name for name, _, _ in JC.REFUSALS}
    for name, data, text in JC.REFUSALS:
        path = str(tmp_path / f"{name}.jpg")
        with open(path, "wb") as fh:
            fh.write(data)
        for mode in ("needed", "always"):
            if name in lifted:
                assert jpeg.read(path, split=mode).split is True
            else:
                with pytest.raises(InvalidOptionError) as e:
                    jpeg.read(path, split=mode)
                assert text in str(e.value) and path in str(e.value), (name, str(e.value))
    # a file without DRI that carries restart markers all the same is refused by its interval count
    data = bytearray(JC.write(17, 33, mode="420", dri=2, seed=5))
    at = data.index(b"\xff\xdd")
    del data[at:at + 6]
    with open(tmp_path / "markers.jpg", "wb") as fh:
        fh.write(bytes(data))
    with pytest.raises(InvalidOptionError, match="restart intervals = "):
        jpeg.read(str(tmp_path / "markers.jpg"), split="needed")


def test_the_options_and_the_status_text(jpeg):
    from shinestacker_amd import DepthMapStack, PyramidStack, _lib
    from shinestacker_amd.errors import ImageLoadError, InvalidOptionError
    for cls in (PyramidStack, DepthMapStack):
        assert cls().jpeg_split is False and cls(jpeg="auto").jpeg_split is False
        assert cls(jpeg="device", jpeg_split=True).jpeg_split is True and cls(jpeg="auto", jpeg_split=True).skipped == []
        with pytest.raises(InvalidOptionError, match="jpeg_split = True"):
            cls(jpeg_split=True)
        with pytest.raises(InvalidOptionError, match="jpeg_split = 1"):
            cls(jpeg="device", jpeg_split="1")
    assert _lib.JPEG_UNSYNCED == S.UNSYNCED == 8
    with pytest.raises(ImageLoadError) as e:
        jpeg.check_status("a.jpg", np.array([8], np.uint32))
    assert "status 8" in str(e.value) and "rounds were too few" in str(e.value)
