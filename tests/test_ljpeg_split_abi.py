"""CPU: the split lossless-JPEG path's entry points are declared, exported and bound; every argument check returns
MI_ERR_INVALID with the argument named before any device call; mi_ljpeg_split_scratch_bytes grows with the span and the layout;
and the stack setter refuses a null handle."""
import ctypes

import numpy as np

NAMES = ("mi_ljpeg_split_scratch_bytes", "mi_raw_ljpeg_split_device", "mi_raw_ljpeg_split", "mi_ljpeg_split_differences_device",
         "mi_ljpeg_split_differences", "mi_stack_set_ljpeg_split")


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert len(hiplib.SIGNATURES["mi_raw_ljpeg_split_device"][1]) == 12 and len(hiplib.SIGNATURES["mi_raw_ljpeg_split"][1]) == 9
    assert hiplib.LJPEG_UNSYNCED == 8 and "rounds" in hiplib.ljpeg_flag_text(8)
    assert hiplib.ljpeg_split_options(False) is None and hiplib.ljpeg_split_options(None) is None
    o = hiplib.ljpeg_split_options({"sub_bytes": 16})
    assert (o.sub_bytes, o.max_rounds) == (16, 0)
    o = hiplib.ljpeg_split_options(True)
    assert (o.sub_bytes, o.max_rounds) == (0, 0)


def _layout(hiplib, h=8, w=12, seg_h=4, bits=12, table_len=0, **kw):
    f = dict(bits=bits, big_endian=0, image_height=h, image_width=w, tiled=0, seg_height=seg_h, seg_width=w, crop_y=0, crop_x=0,
             height=h, width=w, shift=0, table_len=table_len, dtype=hiplib.MI_U8 if bits == 8 else hiplib.MI_U16)
    f.update(kw)
    return hiplib.RawLayoutStruct(*[f[n] for n, _ in hiplib.RawLayoutStruct._fields_])


def _segs(hiplib, n=2, x=6, y=4, ncomp=2, predictor=1, precision=12, scan_off=0, scan_bytes=16):
    segs = np.zeros(n, hiplib.LJPEG_SEG_DTYPE)
    segs["x"], segs["y"], segs["ncomp"], segs["predictor"], segs["precision"] = x, y, ncomp, predictor, precision
    segs["scan_off"], segs["scan_bytes"] = scan_off, scan_bytes
    segs["counts"][:, :, 0] = 1         # one code of one bit: category 0
    return segs


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    span = np.zeros(64, np.uint8)
    out = np.zeros((8, 12), np.uint16)
    plane = np.zeros((2, 4, 12), np.uint16)
    status = np.zeros(2, np.uint32)
    scratch = ctypes.c_void_p(1 << 20)      # (never dereferenced: every call here is refused first)
    good = _segs(hiplib)
    room = np.zeros(good.nbytes + 32, np.uint8)
    odd = room.ctypes.data + (-room.ctypes.data % 16) + 8       # an address that is 8 and not 16-byte aligned

    def expect(rc, msg):
        assert rc == hiplib.MI_ERR_INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    def opt(sub=0, rounds=0):
        return ctypes.byref(hiplib.JpegSplitStruct(sub, rounds))

    def host(sp=span.ctypes.data, nb=span.nbytes, segs=good, L=None, tab=None, o=None, dst=out.ctypes.data, differences=False):
        L = _layout(hiplib) if L is None else L
        sg = None if segs is None else segs.ctypes.data
        if differences:
            return lib.mi_ljpeg_split_differences(0, sp, nb, sg, ctypes.byref(L), o, plane.ctypes.data if dst else None, status.ctypes.data)
        return lib.mi_raw_ljpeg_split(0, sp, nb, sg, ctypes.byref(L), tab, o, dst, status.ctypes.data)

    def device(sp=span.ctypes.data, nb=span.nbytes, sg=good.ctypes.data, L=None, tab=None, o=None, scr=scratch, nscr=1 << 40,
               dst=out.ctypes.data, st=status.ctypes.data, differences=False):
        L = _layout(hiplib) if L is None else L
        if differences:
            return lib.mi_ljpeg_split_differences_device(0, None, sp, nb, sg, ctypes.byref(L), o, scr, nscr, dst, st)
        return lib.mi_raw_ljpeg_split_device(0, None, sp, nb, sg, ctypes.byref(L), tab, o, scr, nscr, dst, st)

    for differences in (False, True):
        for call in (host, device):
            kw = dict(differences=differences)
            expect(call(sp=None, **kw), b"null span")
            expect(call(**{"segs" if call is host else "sg": None}, **kw), b"null segs")
            expect(call(dst=None, **kw), b"null output")
            expect(call(nb=0, **kw), b"span_bytes must be in [1, 2^32)")
            expect(call(L=_layout(hiplib, bits=11), **kw), b"layout bits must be 8, 10, 12, 14 or 16")
            expect(call(L=_layout(hiplib, seg_width=5), **kw), b"layout seg_width of strips must be image_width")
            expect(call(L=_layout(hiplib, crop_y=1), **kw), b"lies outside the")
            expect(call(L=_layout(hiplib, shift=16), **kw), b"layout shift must be in [0, 15]")
            expect(call(o=opt(sub=24), **kw), b"split sub_bytes must be 0, 8, 16, 32, 64 or 128 (got 24)")
            expect(call(L=_layout(hiplib, h=1 << 17, w=1 << 15, seg_h=1 << 17, height=8, width=12), **kw), b"below 2^32 for the split path")
        if not differences:
            expect(host(L=_layout(hiplib, table_len=16)), b"layout table_len is 16 and the table is null")
            expect(device(L=_layout(hiplib, table_len=16)), b"layout table_len is 16 and the table is null")
        # the descriptors, where they lie in host memory: mi_raw_ljpeg's checks
        kw = dict(differences=differences)
        expect(host(segs=_segs(hiplib, ncomp=3), **kw), b"segs[0].ncomp must be 1 or 2 (got 3)")
        expect(host(segs=_segs(hiplib, predictor=8), **kw), b"segs[0].predictor must be in [1, 7] (got 8)")
        expect(host(segs=_segs(hiplib, precision=13), **kw), b"segs[0].precision must be in [2, layout bits = 12] (got 13)")
        expect(host(segs=_segs(hiplib, x=5), **kw), b"does not match its segment")
        expect(host(segs=_segs(hiplib, scan_off=60), **kw), b"outside the span of 64 bytes")
        # the scratch and the alignments of the device forms
        expect(device(scr=None, **kw), b"null scratch")
        need = ctypes.c_size_t(0)
        L = _layout(hiplib)
        assert lib.mi_ljpeg_split_scratch_bytes(ctypes.byref(L), span.nbytes, None, ctypes.byref(need)) == 0
        expect(device(nscr=64, **kw), b"scratch_bytes must be >= %d (got 64)" % need.value)     # (the size needed, by name)
        expect(device(nscr=need.value - 1, **kw), b"scratch_bytes must be >= %d" % need.value)
        expect(device(scr=ctypes.c_void_p((1 << 20) + 128), **kw), b"dev_scratch must be 256-byte aligned")
        expect(device(sp=span.ctypes.data + 1, **kw), b"dev_span must be 4-byte aligned")
        expect(device(sg=odd, **kw), b"dev_segs must be 16-byte aligned")
        expect(device(st=status.ctypes.data + 2, **kw), b"dev_status must be 4-byte aligned")
        expect(device(dst=out.ctypes.data + 1, **kw), b"dev_plane must be 2-byte aligned" if differences else b"dev_out must be aligned to its samples")


def test_scratch_bytes_checks_and_grows_with_the_span_and_the_layout(hiplib):
    lib = hiplib.load()
    need = ctypes.c_size_t(0)

    def size(L, nb, o=None):
        assert lib.mi_ljpeg_split_scratch_bytes(ctypes.byref(L), nb, o, ctypes.byref(need)) == 0, lib.mi_last_error()
        return need.value
    L = _layout(hiplib)
    assert lib.mi_ljpeg_split_scratch_bytes(None, 64, None, ctypes.byref(need)) == hiplib.MI_ERR_INVALID and b"null layout" in lib.mi_last_error()
    assert lib.mi_ljpeg_split_scratch_bytes(ctypes.byref(L), 64, None, None) == hiplib.MI_ERR_INVALID and b"null bytes" in lib.mi_last_error()
    assert lib.mi_ljpeg_split_scratch_bytes(ctypes.byref(L), 0, None, ctypes.byref(need)) == hiplib.MI_ERR_INVALID
    bad = hiplib.JpegSplitStruct(7, 0)
    assert lib.mi_ljpeg_split_scratch_bytes(ctypes.byref(L), 64, ctypes.byref(bad), ctypes.byref(need)) == hiplib.MI_ERR_INVALID
    spans = [size(L, nb) for nb in (1, 64, 4096, 1 << 16, 1 << 20, 1 << 26)]
    assert spans == sorted(spans) and spans[0] > 0 and spans[-1] > spans[0]
    layouts = [size(_layout(hiplib, h=h, w=w, seg_h=sh), 1 << 16) for h, w, sh in ((8, 12, 8), (8, 12, 4), (64, 12, 4), (64, 96, 4), (640, 960, 4))]
    assert layouts == sorted(layouts) and layouts[-1] > layouts[0]
    for sub in (8, 16, 32, 64, 128):       # shorter subsequences, more lanes
        o = hiplib.JpegSplitStruct(sub, 0)
        assert size(L, 1 << 20, ctypes.byref(o)) >= size(L, 1 << 20)
    few, many = hiplib.JpegSplitStruct(8, 1), hiplib.JpegSplitStruct(8, 0xFFFFFFFF)
    assert size(L, 1 << 20, ctypes.byref(few)) <= size(L, 1 << 20, ctypes.byref(many))


def test_the_stack_setter_refuses_a_null_handle(hiplib):
    lib = hiplib.load()
    assert lib.mi_stack_set_ljpeg_split(None, None) == hiplib.MI_ERR_INVALID and b"null handle" in lib.mi_last_error()
    o = hiplib.JpegSplitStruct(0, 0)
    assert lib.mi_stack_set_ljpeg_split(None, ctypes.byref(o)) == hiplib.MI_ERR_INVALID and b"null handle" in lib.mi_last_error()
