"""CPU: the split JPEG decoder's entry points are declared, exported and bound, mi_jpeg_split_t equals its ctypes mirror,
mi_jpeg_t and MI_ABI_VERSION are what they were, and every argument check returns MI_ERR_INVALID with the argument named
before any device call -- the checks of the serial entry points, with dri allowed up to the MCU count, and those of the
options and the scratch."""
import ctypes
import re

import numpy as np

from test_develop_abi import HEADER

NAMES = ("mi_jpeg_split_scratch_bytes", "mi_jpeg_split_coefficients_device", "mi_jpeg_split_coefficients", "mi_jpeg_split_decode_device",
         "mi_jpeg_split_decode")


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert hiplib.load().mi_abi_version() == 1
    assert [len(hiplib.SIGNATURES[n][1]) for n in NAMES] == [4, 11, 8, 11, 8]
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for decl in ("typedef struct { uint32_t sub_bytes; uint32_t max_rounds; } mi_jpeg_split_t;",
                 "int mi_jpeg_split_scratch_bytes(const mi_jpeg_t* jpeg, size_t span_bytes, const mi_jpeg_split_t* opt, size_t* bytes);",
                 "int mi_jpeg_split_coefficients_device(int device, void* stream, const void* dev_span, size_t span_bytes, "
                 "const uint32_t* dev_offsets, const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt, void* dev_scratch, size_t scratch_bytes, "
                 "int16_t* dev_coef, uint32_t* dev_status);",
                 "int mi_jpeg_split_coefficients(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, "
                 "const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt, int16_t* host_coef, uint32_t* status_out);",
                 "int mi_jpeg_split_decode_device(int device, void* stream, const void* dev_span, size_t span_bytes, "
                 "const uint32_t* dev_offsets, const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt, void* dev_scratch, size_t scratch_bytes, "
                 "uint8_t* dev_out, uint32_t* dev_status);",
                 "int mi_jpeg_split_decode(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, "
                 "const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt, uint8_t* host_out, uint32_t* status_out);"):
        assert decl in flat, decl
    assert re.search(r"#define MI_JPEG_UNSYNCED 8u\b", text) and re.search(r"#define MI_JPEG_MAX_DRI 8192\b", text)
    assert "} mi_jpeg_t;                /* 1392 bytes */" in text and ctypes.sizeof(hiplib.JpegStruct) == 1392
    mine = hiplib.JpegSplitStruct
    assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == [("sub_bytes", 0, 4), ("max_rounds", 4, 4)]
    assert ctypes.sizeof(mine) == 8 and hiplib.JPEG_UNSYNCED == 8


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    span = np.zeros(64, np.uint8)
    offsets = np.array([0, 10, 20], np.uint32)
    coef = np.zeros(6 * 64 + 64, np.int16)
    out = np.zeros((8, 16, 3), np.uint8)
    status = np.zeros(2, np.uint32)
    sp, fp, cp, op, stp = (a.ctypes.data for a in (span, offsets, coef, out, status))
    cp = (cp + 15) & ~15

    def desc(**bad):
        # 8 x 16 in 4:4:4: two MCUs, one per interval; a one-code DC table and a one-code AC table
        d = hiplib.JpegStruct()
        d.width, d.height, d.ncomp, d.hmax, d.vmax, d.dri, d.n_intervals = 16, 8, 3, 1, 1, 1, 2
        for c in range(3):
            d.tq[c], d.td[c], d.ta[c] = (0, 0, 0) if c == 0 else (1, 1, 1)
        for t in range(4):
            d.counts[t][0] = 1
            for k in range(64):
                d.quant[t][k] = 1
        for key, v in bad.items():
            if key in ("tq", "td", "ta"):
                getattr(d, key)[2] = v
            elif key == "counts":
                for i, n in enumerate(v[1]):
                    d.counts[v[0]][i] = n
            elif key == "value":
                d.values[v[0]][v[1]] = v[2]
            elif key == "quant":
                d.quant[v[0]][v[1]] = v[2]
            else:
                setattr(d, key, v)
        return ctypes.byref(d)

    def opt(sub=0, rounds=0):
        o = hiplib.JpegSplitStruct()
        o.sub_bytes, o.max_rounds = sub, rounds
        return ctypes.byref(o)

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    BIG = 1 << 24
    calls = (lambda s, n, f, d, o, q=None: lib.mi_jpeg_split_coefficients_device(0, None, s, n, f, d, q, 256, BIG, o if o is None else cp, None),
             lambda s, n, f, d, o, q=None: lib.mi_jpeg_split_coefficients(0, s, n, f, d, q, o if o is None else cp, stp),
             lambda s, n, f, d, o, q=None: lib.mi_jpeg_split_decode_device(0, None, s, n, f, d, q, 256, BIG, o, None),
             lambda s, n, f, d, o, q=None: lib.mi_jpeg_split_decode(0, s, n, f, d, q, o, stp))
    for call in calls:
        expect(call(None, 64, fp, desc(), op), b"null span")
        expect(call(sp, 64, None, desc(), op), b"null offsets")
        expect(call(sp, 64, fp, None, op), b"null jpeg")
        expect(call(sp, 64, fp, desc(), None), b"null output")
        expect(call(sp, 0, fp, desc(), op), b"span_bytes must be in [1, 2^32) (got 0)")
        expect(call(sp, 1 << 32, fp, desc(), op), b"span_bytes must be in [1, 2^32) (got 4294967296)")
        expect(call(sp, 64, fp, desc(width=0), op), b"jpeg width and height must be in [1, 65535] (got 0 x 8)")
        expect(call(sp, 64, fp, desc(height=65536), op), b"jpeg width and height must be in [1, 65535] (got 16 x 65536)")
        expect(call(sp, 64, fp, desc(ncomp=2), op), b"jpeg ncomp must be 1 or 3 (got 2)")
        expect(call(sp, 64, fp, desc(hmax=1, vmax=2), op), b"jpeg hmax, vmax must be (1,1), or (2,1) or (2,2) at ncomp 3 (got (1,2))")
        expect(call(sp, 64, fp, desc(hmax=4), op), b"(got (4,1))")
        expect(call(sp, 64, fp, desc(ncomp=1, hmax=2), op), b"(got (2,1))")
        # dri: 1 .. the MCU count (2 here), whatever MI_JPEG_MAX_DRI says
        expect(call(sp, 64, fp, desc(dri=0), op), b"jpeg dri must be in [1, 2] (got 0)")
        expect(call(sp, 64, fp, desc(dri=3, n_intervals=1), op), b"jpeg dri must be in [1, 2] (got 3)")
        expect(call(sp, 64, fp, desc(dri=8193, n_intervals=1), op), b"jpeg dri must be in [1, 2] (got 8193)")
        expect(call(sp, 64, fp, desc(n_intervals=3), op), b"jpeg n_intervals must be ceil(2 MCUs / dri 1) = 2 (got 3)")
        expect(call(sp, 64, fp, desc(dri=2), op), b"jpeg n_intervals must be ceil(2 MCUs / dri 2) = 1 (got 2)")
        expect(call(sp, 64, fp, desc(tq=4), op), b"jpeg tq[2] must be in [0, 3] (got 4)")
        expect(call(sp, 64, fp, desc(td=2), op), b"jpeg td[2] must be 0 or 1 (got 2)")
        expect(call(sp, 64, fp, desc(ta=3), op), b"jpeg ta[2] must be 0 or 1 (got 3)")
        expect(call(sp, 64, fp, desc(quant=(1, 9, 0)), op), b"jpeg quant[1][9] must be >= 1")
        expect(call(sp, 64, fp, desc(counts=(2, [3])), op), b"jpeg counts[2] overflow the code space at length 1")
        expect(call(sp, 64, fp, desc(counts=(1, [0])), op), b"jpeg counts[1] must sum to 1 .. 256 (got 0)")
        expect(call(sp, 64, fp, desc(counts=(2, [0] * 8 + [200, 57])), op), b"jpeg counts[2] must sum to 1 .. 256 (got 257)")
        expect(call(sp, 64, fp, desc(value=(0, 0, 16)), op), b"jpeg values[0][0] must be <= 15 in a DC table (got 16)")
        for sub in (1, 7, 12, 24, 256, 129):
            expect(call(sp, 64, fp, desc(), op, opt(sub)), b"split sub_bytes must be 0, 8, 16, 32, 64 or 128 (got %d)" % sub)
    # the host forms see the offsets
    for call in (calls[1], calls[3]):
        bad = np.array([0, 10, 65], np.uint32)
        expect(call(sp, 64, bad.ctypes.data, desc(), op), b"offsets[2] = 65 lies outside the span of 64 bytes")
        bad = np.array([12, 10, 20], np.uint32)
        expect(call(sp, 64, bad.ctypes.data, desc(), op), b"offsets[1] = 10 lies in front of offsets[0] = 12")
    # the sizes: the planes of the serial decoder's scratch, then the passes' own; more lanes, more rounds, more bytes
    n = ctypes.c_size_t(7)
    size = lib.mi_jpeg_split_scratch_bytes
    expect(size(None, 64, None, ctypes.byref(n)), b"null jpeg")
    expect(size(desc(ncomp=4), 64, None, ctypes.byref(n)), b"jpeg ncomp must be 1 or 3 (got 4)")
    expect(size(desc(), 0, None, ctypes.byref(n)), b"span_bytes must be in [1, 2^32) (got 0)")
    expect(size(desc(), 64, opt(9), ctypes.byref(n)), b"split sub_bytes must be 0, 8, 16, 32, 64 or 128 (got 9)")
    expect(size(desc(), 64, None, None), b"null bytes")
    assert n.value == 7
    sizes = {}
    for sub, rounds, nbytes in ((0, 0, 64), (128, 8, 64), (8, 0, 64), (8, 0, 1 << 20), (8, 1, 1 << 20), (8, 0xFFFFFFFF, 1 << 20)):
        assert size(desc(), nbytes, opt(sub, rounds), ctypes.byref(n)) == hiplib.MI_OK
        sizes[(sub, rounds, nbytes)] = n.value
        assert n.value > 6 * 192 and n.value % 64 == 0
    assert sizes[(0, 0, 64)] == sizes[(128, 8, 64)] and sizes[(8, 0, 1 << 20)] > sizes[(8, 0, 64)]
    assert sizes[(8, 1, 1 << 20)] <= sizes[(8, 0, 1 << 20)] <= sizes[(8, 0xFFFFFFFF, 1 << 20)]
    assert size(desc(dri=2, n_intervals=1), 64, None, ctypes.byref(n)) == hiplib.MI_OK      # one interval of every MCU
    # the device forms want buffers their accesses can take
    need = sizes[(0, 0, 64)]
    for dev, o in ((lib.mi_jpeg_split_coefficients_device, cp), (lib.mi_jpeg_split_decode_device, op)):
        expect(dev(0, None, sp, 64, fp, desc(), None, None, BIG, o, None), b"null scratch")
        expect(dev(0, None, sp, 64, fp, desc(), None, 256, need - 1, o, None), b"scratch_bytes must be >= %d (got %d)" % (need, need - 1))
        expect(dev(0, None, sp, 64, fp, desc(), None, 384, BIG, o, None), b"dev_scratch must be 256-byte aligned")
        expect(dev(0, None, sp + 1, 63, fp, desc(), None, 256, BIG, o, None), b"dev_span must be 4-byte aligned")
        expect(dev(0, None, sp, 64, fp + 2, desc(), None, 256, BIG, o, None), b"dev_offsets must be 4-byte aligned")
        expect(dev(0, None, sp, 64, fp, desc(), None, 256, BIG, o, stp + 2), b"dev_status must be 4-byte aligned")
    expect(lib.mi_jpeg_split_coefficients_device(0, None, sp, 64, fp, desc(), None, 256, BIG, cp + 2, None), b"dev_coef must be 16-byte aligned")
    # the serial entry points keep their limit
    expect(lib.mi_jpeg_decode(0, sp, 64, fp, desc(dri=8193, n_intervals=1), op, stp), b"jpeg dri must be in [1, 8192] (got 8193)")
    assert not out.any() and not status.any() and not coef.any()
    if hiplib.device_count() == 0:      # a valid call gets as far as asking for a device
        rc = lib.mi_jpeg_split_decode(0, sp, 64, fp, desc(), None, op, stp)
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
