"""CPU: the lossless-JPEG entry points of the C boundary are declared, exported and bound, mi_ljpeg_seg_t as the header declares
it equals its ctypes mirror and its NumPy record, MI_ABI_VERSION and mi_raw_layout_t are what they were, and every argument
check returns MI_ERR_INVALID with the argument named before any device call."""
import ctypes
import re

import numpy as np

from test_develop_abi import HEADER, header_struct

NAMES = ("mi_raw_ljpeg_device", "mi_raw_ljpeg", "mi_stack_push_ljpeg", "mi_stack_ljpeg_status")
LAYOUT_FIELDS = ["bits", "big_endian", "image_height", "image_width", "tiled", "seg_height", "seg_width", "crop_y", "crop_x", "height",
                 "width", "shift", "table_len", "dtype"]
# (member, C type, dimensions, offset, bytes)
SEG = [("scan_off", "uint32_t", (), 0, 4), ("scan_bytes", "uint32_t", (), 4, 4), ("x", "int32_t", (), 8, 4), ("y", "int32_t", (), 12, 4),
       ("ncomp", "uint8_t", (), 16, 1), ("predictor", "uint8_t", (), 17, 1), ("precision", "uint8_t", (), 18, 1),
       ("reserved", "uint8_t", (), 19, 1), ("counts", "uint8_t", (2, 16), 20, 32), ("values", "uint8_t", (2, 17), 52, 34),
       ("pad", "uint8_t", (10,), 86, 10)]


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert hiplib.load().mi_abi_version() == 1
    assert [len(hiplib.SIGNATURES[n][1]) for n in NAMES] == [9, 8, 12, 2]
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for decl in ("int mi_raw_ljpeg_device(int device, void* stream, const void* dev_span, size_t span_bytes, "
                 "const mi_ljpeg_seg_t* dev_segs, const mi_raw_layout_t* layout, const uint16_t* dev_table, void* dev_out, "
                 "uint32_t* dev_status);",
                 "int mi_raw_ljpeg(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs, "
                 "const mi_raw_layout_t* layout, const uint16_t* host_table, void* host_out, uint32_t* status_out);",
                 "int mi_stack_push_ljpeg(mi_stack_t* s, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs, "
                 "const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_cfa_t* cfa, const mi_calib_t* calib, "
                 "const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned);",
                 "int mi_stack_ljpeg_status(mi_stack_t* s, uint32_t* flags);"):
        assert decl in flat, decl
    assert re.search(r"#define MI_ABI_VERSION 1\b", text)
    assert header_struct("mi_raw_layout") == [(n, "int32_t", 1) for n in LAYOUT_FIELDS]        # unchanged
    for name, value in (("MI_LJPEG_NOCODE", "1u"), ("MI_LJPEG_OVERRUN", "2u"), ("MI_LJPEG_UNDECODED", "4u"), ("MI_LJPEG_MAX_LINE", "24576")):
        assert re.search(r"#define %s %s\b" % (name, value), text), name
    assert (hiplib.LJPEG_NOCODE, hiplib.LJPEG_OVERRUN, hiplib.LJPEG_UNDECODED, hiplib.LJPEG_MAX_LINE) == (1, 2, 4, 24576)


def test_segment_struct_layout(hiplib):
    text = open(HEADER).read()
    body = text[text.index("typedef struct mi_ljpeg_seg {"):text.index("} mi_ljpeg_seg_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    declared = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.match(r"(\w+)\s+(\w+)((?:\[\d+\])*)$", decl.strip())
            declared.append((m.group(2), m.group(1), tuple(int(d) for d in re.findall(r"\[(\d+)\]", m.group(3)))))
    assert declared == [(n, t, dims) for n, t, dims, _, _ in SEG]
    mine = hiplib.LjpegSeg
    assert [f[0] for f in mine._fields_] == [s[0] for s in SEG]
    for n, _, _, off, size in SEG:
        assert (getattr(mine, n).offset, getattr(mine, n).size) == (off, size), n
        assert hiplib.LJPEG_SEG_DTYPE.fields[n][1] == off and hiplib.LJPEG_SEG_DTYPE.fields[n][0].itemsize == size, n
    assert ctypes.sizeof(mine) == hiplib.LJPEG_SEG_DTYPE.itemsize == 96 and 96 % 16 == 0


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    U8, U16 = hiplib.MI_U8, hiplib.MI_U16
    span = np.zeros(256, np.uint8)
    table = np.zeros(16, np.uint16)
    out = np.zeros((4, 6), np.uint16)
    status = np.zeros(4, np.uint32)
    sp, tp, op, stp = span.ctypes.data, table.ctypes.data, out.ctypes.data, status.ctypes.data

    def segs(n=1, **bad):
        # 4 x 6 in one strip: two components of 3 samples a line, a one-code table each
        a = np.zeros(n, hiplib.LJPEG_SEG_DTYPE)
        a["scan_off"], a["scan_bytes"], a["x"], a["y"], a["ncomp"], a["predictor"], a["precision"] = 40, 24, 3, 4, 2, 1, 12
        a["counts"][:, :, 0] = 1
        for key, v in bad.items():
            if key == "counts0":
                a["counts"][-1, 0, :] = v
            elif key == "values0":
                a["values"][-1, 0, :len(v)] = v
            else:
                a[key][-1] = v
        return a

    def layout(**bad):
        v = dict(bits=12, big_endian=0, image_height=4, image_width=6, tiled=0, seg_height=4, seg_width=6, crop_y=0, crop_x=0,
                 height=4, width=6, shift=4, table_len=0, dtype=U16)
        v.update(bad)
        return ctypes.byref(hiplib.RawLayoutStruct(*[v[n] for n in LAYOUT_FIELDS]))

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    good = segs()
    gp = good.ctypes.data
    calls = (lambda s, n, g, L, t, o: lib.mi_raw_ljpeg_device(0, None, s, n, g, L, t, o, None),
             lambda s, n, g, L, t, o: lib.mi_raw_ljpeg(0, s, n, g, L, t, o, stp))
    for call in calls:
        # raw_layout_check, reused: the descriptors stand where the offsets did
        expect(call(None, 256, gp, layout(), None, op), b"null span")
        expect(call(sp, 256, None, layout(), None, op), b"null segs")
        expect(call(sp, 256, gp, None, None, op), b"null layout")
        expect(call(sp, 256, gp, layout(), None, None), b"null output")
        expect(call(sp, 256, gp, layout(bits=11), None, op), b"layout bits must be 8, 10, 12, 14 or 16 (got 11)")
        expect(call(sp, 256, gp, layout(dtype=U8), None, op), b"layout dtype must be MI_U8 for 8 bits and MI_U16 otherwise")
        expect(call(sp, 256, gp, layout(image_height=0), None, op), b"layout image_height and image_width must be >= 1")
        expect(call(sp, 256, gp, layout(seg_width=5), None, op), b"layout seg_width of strips must be image_width")
        expect(call(sp, 256, gp, layout(crop_x=1), None, op), b"lies outside the 6x4 image")
        expect(call(sp, 0, gp, layout(), None, op), b"span_bytes must be in [1, 2^32)")
        expect(call(sp, 1 << 32, gp, layout(), None, op), b"span_bytes must be in [1, 2^32) (got 4294967296)")
        expect(call(sp, 256, gp, layout(shift=16), None, op), b"layout shift must be in [0, 15]")
        expect(call(sp, 256, gp, layout(table_len=16), None, op), b"layout table_len is 16 and the table is null")
        expect(call(sp, 256, gp, layout(table_len=65537), tp, op), b"layout table_len must be in [0, 65536] (got 65537)")
    # the host forms see the descriptors
    host = calls[1]

    def bad(msg, L=None, n=1, span_bytes=256, **kw):
        a = segs(n, **kw)
        expect(host(sp, span_bytes, a.ctypes.data, L or layout(), None, op), msg)
    bad(b"segs[0].ncomp must be 1 or 2 (got 3)", ncomp=3)
    bad(b"segs[0].ncomp must be 1 or 2 (got 0)", ncomp=0)
    bad(b"segs[0].predictor must be in [1, 7] (got 0)", predictor=0)
    bad(b"segs[0].predictor must be in [1, 7] (got 8)", predictor=8)
    bad(b"segs[0].precision must be in [2, layout bits = 12] (got 13)", precision=13)
    bad(b"segs[0].precision must be in [2, layout bits = 12] (got 1)", precision=1)
    bad(b"segs[0]: a frame of 4 lines of 2 x 2 samples does not match its segment of 4 x 6", x=2)
    bad(b"segs[0]: a frame of 3 lines of 3 x 2 samples does not match its segment of 4 x 6", y=3)
    bad(b"segs[0]: a frame of 4 lines of 3 x 1 samples does not match its segment of 4 x 6", ncomp=1)
    bad(b"segs[0].counts[0] overflow the code space at length 1", counts0=[3] + [0] * 15)
    bad(b"segs[0].counts[0] overflow the code space at length 2", counts0=[1, 3] + [0] * 14)
    bad(b"segs[0].counts[0] must sum to 1 .. 17 (got 0)", counts0=[0] * 16)
    bad(b"segs[0].counts[0] must sum to 1 .. 17 (got 18)", counts0=[0, 0, 0, 0, 18] + [0] * 11)
    bad(b"segs[0].values[0][1] must be <= 16 (got 17)", counts0=[0, 2] + [0] * 14, values0=[3, 17])
    bad(b"segs[0].scan_off = 40: the data ends at 64, outside the span of 63 bytes", span_bytes=63)
    bad(b"segs[0].scan_off = 250: the data ends at 274, outside the span of 256 bytes", scan_off=250)
    # strips of 1 row: the fourth descriptor is the one named; the last strip's rows
    a = segs(4, predictor=9)
    a["y"] = 1
    expect(host(sp, 256, a.ctypes.data, layout(seg_height=1), None, op), b"segs[3].predictor must be in [1, 7] (got 9)")
    a = segs(2)
    a["y"] = (3, 3)
    expect(host(sp, 256, a.ctypes.data, layout(seg_height=3), None, op), b"segs[1]: a frame of 3 lines of 3 x 2 samples does not match its segment of 1 x 6")
    # a predictor that keeps the line above, wider than the line buffer
    wide = dict(image_width=24578, seg_width=24578, width=24578, image_height=1, seg_height=1, height=1)
    a = segs(1, x=12289, y=1, predictor=2)
    big = np.zeros(24578, np.uint16)
    expect(lib.mi_raw_ljpeg(0, sp, 256, a.ctypes.data, layout(**wide), None, big.ctypes.data, None),
           b"segs[0].predictor 2 keeps the line above: layout seg_width must be <= 24576 for it (got 24578)")
    # the device form wants buffers its accesses can take
    expect(lib.mi_raw_ljpeg_device(0, None, sp + 1, 255, gp, layout(), None, op, None), b"dev_span must be 4-byte aligned")
    expect(lib.mi_raw_ljpeg_device(0, None, sp, 256, gp + 4, layout(), None, op, None), b"dev_segs must be 16-byte aligned")
    expect(lib.mi_raw_ljpeg_device(0, None, sp, 256, gp, layout(), None, op + 1, None), b"dev_out must be aligned to its samples")
    expect(lib.mi_raw_ljpeg_device(0, None, sp, 256, gp, layout(), None, op, stp + 2), b"dev_status must be 4-byte aligned")
    # the push and the status: the handle first
    expect(lib.mi_stack_push_ljpeg(None, sp, 256, gp, layout(), None, None, None, None, None, 0, 0), b"null")
    flags = ctypes.c_uint32(7)
    expect(lib.mi_stack_ljpeg_status(None, ctypes.byref(flags)), b"null")
    assert not out.any() and not status.any()
    if hiplib.device_count() == 0:      # a valid call gets as far as asking for a device
        rc = lib.mi_raw_ljpeg(0, sp, 256, gp, layout(), None, op, stp)
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
