"""CPU: the packed-raw entry points of the C boundary are declared, exported and bound, mi_raw_layout_t as the header declares
it equals its ctypes mirror, and every argument check returns MI_ERR_INVALID with the argument named before any device call."""
import ctypes
import re

import numpy as np

from test_develop_abi import HEADER, header_struct

NAMES = ("mi_raw_unpack_device", "mi_raw_unpack", "mi_stack_push_packed")
FIELDS = ["bits", "big_endian", "image_height", "image_width", "tiled", "seg_height", "seg_width", "crop_y", "crop_x", "height",
          "width", "shift", "table_len", "dtype"]


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert hiplib.load().mi_abi_version() == 1
    assert [len(hiplib.SIGNATURES[n][1]) for n in NAMES] == [8, 7, 12]
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    for decl in ("int mi_raw_unpack_device(int device, void* stream, const void* dev_span, size_t span_bytes, "
                 "const uint32_t* dev_seg_offsets, const mi_raw_layout_t* layout, const uint16_t* dev_table, void* dev_out);",
                 "int mi_raw_unpack(int device, const void* host_span, size_t span_bytes, const uint32_t* seg_offsets, "
                 "const mi_raw_layout_t* layout, const uint16_t* host_table, void* host_out);",
                 "int mi_stack_push_packed(mi_stack_t* s, const void* host_span, size_t span_bytes, const uint32_t* seg_offsets, "
                 "const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_cfa_t* cfa, const mi_calib_t* calib, "
                 "const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned);"):
        assert decl in flat, decl
    assert re.search(r"#define MI_ABI_VERSION 1\b", open(HEADER).read())


def test_raw_layout_struct_layout(hiplib):
    fields = header_struct("mi_raw_layout")
    assert fields == [(n, "int32_t", 1) for n in FIELDS]
    mine = hiplib.RawLayoutStruct
    assert [f[0] for f in mine._fields_] == FIELDS
    for i, n in enumerate(FIELDS):
        assert getattr(mine, n).offset == 4 * i and getattr(mine, n).size == 4, n
    assert ctypes.sizeof(mine) == 56


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    U8, U16 = hiplib.MI_U8, hiplib.MI_U16
    span = np.zeros(64, np.uint8)
    seg = np.zeros(4, np.uint32)
    table = np.zeros(16, np.uint16)
    out = np.zeros((4, 6), np.uint16)
    sp, gp, tp, op = span.ctypes.data, seg.ctypes.data, table.ctypes.data, out.ctypes.data

    def layout(**bad):
        # 12 bits, 4 x 6 in one strip: 9 bytes a row, 36 bytes
        v = dict(bits=12, big_endian=0, image_height=4, image_width=6, tiled=0, seg_height=4, seg_width=6, crop_y=0, crop_x=0,
                 height=4, width=6, shift=4, table_len=0, dtype=U16)
        v.update(bad)
        return ctypes.byref(hiplib.RawLayoutStruct(*[v[n] for n in FIELDS]))

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    calls = (lambda s, n, g, L, t, o: lib.mi_raw_unpack_device(0, None, s, n, g, L, t, o),
             lambda s, n, g, L, t, o: lib.mi_raw_unpack(0, s, n, g, L, t, o))
    for call in calls:
        expect(call(None, 64, gp, layout(), None, op), b"null span")
        expect(call(sp, 64, None, layout(), None, op), b"null seg_offsets")
        expect(call(sp, 64, gp, None, None, op), b"null layout")
        expect(call(sp, 64, gp, layout(), None, None), b"null output")
        for bits in (0, 9, 11, 13, 15, 17, 32):
            expect(call(sp, 64, gp, layout(bits=bits), None, op), b"layout bits must be 8, 10, 12, 14 or 16 (got %d)" % bits)
        expect(call(sp, 64, gp, layout(dtype=U8), None, op), b"layout dtype must be MI_U8 for 8 bits and MI_U16 otherwise")
        expect(call(sp, 64, gp, layout(bits=8), None, op), b"layout dtype must be MI_U8 for 8 bits and MI_U16 otherwise")
        expect(call(sp, 64, gp, layout(dtype=hiplib.MI_F32), None, op), b"layout dtype must be")
        expect(call(sp, 64, gp, layout(image_height=0), None, op), b"layout image_height and image_width must be >= 1")
        expect(call(sp, 64, gp, layout(image_width=-3), None, op), b"layout image_height and image_width must be >= 1")
        expect(call(sp, 64, gp, layout(seg_height=0), None, op), b"layout seg_height and seg_width must be >= 1")
        expect(call(sp, 64, gp, layout(seg_width=5), None, op), b"layout seg_width of strips must be image_width")
        expect(call(sp, 64, gp, layout(height=0), None, op), b"layout height and width must be >= 1")
        expect(call(sp, 64, gp, layout(width=0), None, op), b"layout height and width must be >= 1")
        expect(call(sp, 64, gp, layout(crop_y=-1), None, op), b"layout crop")
        expect(call(sp, 64, gp, layout(crop_x=1), None, op), b"lies outside the 6x4 image")
        expect(call(sp, 64, gp, layout(crop_y=1), None, op), b"lies outside the 6x4 image")
        expect(call(sp, 64, gp, layout(height=5), None, op), b"lies outside the 6x4 image")
        big = dict(image_height=65536, image_width=32768, seg_height=65536, seg_width=32768, height=65536, width=32768)
        expect(call(sp, 64, gp, layout(**big), None, op), b"layout height x width too large")
        expect(call(sp, 0, gp, layout(), None, op), b"span_bytes must be in [1, 2^32)")
        expect(call(sp, 1 << 32, gp, layout(), None, op), b"span_bytes must be in [1, 2^32) (got 4294967296)")
        expect(call(sp, 64, gp, layout(shift=-1), None, op), b"layout shift must be in [0, 15]")
        expect(call(sp, 64, gp, layout(shift=16), None, op), b"layout shift must be in [0, 15]")
        expect(call(sp, 64, gp, layout(table_len=-1), None, op), b"layout table_len must be in [0, 65536]")
        expect(call(sp, 64, gp, layout(table_len=65537), tp, op), b"layout table_len must be in [0, 65536] (got 65537)")
        expect(call(sp, 64, gp, layout(table_len=16), None, op), b"layout table_len is 16 and the table is null")
        expect(call(sp, 64, gp, layout(bits=8, dtype=U8, table_len=16), tp, op), b"layout table_len must be 0 for 8-bit samples")
    # the host forms see the offsets: a segment that ends outside the span
    host = calls[1]
    expect(host(sp, 35, gp, layout(), None, op), b"seg_offsets[0] = 0: the segment ends at 36, outside the span of 35 bytes")
    seg[0] = 29
    expect(host(sp, 64, gp, layout(), None, op), b"seg_offsets[0] = 29: the segment ends at 65, outside the span of 64 bytes")
    seg[:] = (0, 9, 18, 28)     # strips of one row, the last a byte too far
    expect(host(sp, 36, gp, layout(seg_height=1), None, op), b"seg_offsets[3] = 28: the segment ends at 37")
    seg[:] = 0                  # tiles are stored whole: 2 x 2 tiles of 3 x 4 on 4 x 6 take 3 rows of 6 bytes each
    expect(host(sp, 17, gp, layout(tiled=1, seg_height=3, seg_width=4), None, op), b"the segment ends at 18, outside the span of 17 bytes")
    # the device form wants buffers its vector accesses can take
    expect(lib.mi_raw_unpack_device(0, None, sp + 1, 63, gp, layout(), None, op), b"dev_span must be 4-byte aligned")
    expect(lib.mi_raw_unpack_device(0, None, sp, 64, gp, layout(), None, op + 1), b"dev_out must be aligned to its samples")
    # the push: the handle first, and nothing of a span is looked at without one
    expect(lib.mi_stack_push_packed(None, sp, 64, gp, layout(), None, None, None, None, None, 0, 0), b"null")
    assert not out.any()
    if hiplib.device_count() == 0:      # a valid call gets as far as asking for a device
        rc = lib.mi_raw_unpack(0, sp, 64, gp, layout(), None, op)
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
