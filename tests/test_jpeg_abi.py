"""CPU: the JPEG entry points of the C boundary are declared, exported and bound, mi_jpeg_t as the header declares it equals
its ctypes mirror, MI_ABI_VERSION is what it was, and every argument check returns MI_ERR_INVALID with the argument named
before any device call -- null handles and pointers included."""
import ctypes
import re

import numpy as np

from test_develop_abi import HEADER

NAMES = ("mi_jpeg_coef_count", "mi_jpeg_scratch_bytes", "mi_jpeg_coefficients_device", "mi_jpeg_coefficients", "mi_jpeg_decode_device",
         "mi_jpeg_decode")
# (member, C type, dimensions, offset, bytes)
FIELDS = [("width", "int32_t", (), 0, 4), ("height", "int32_t", (), 4, 4), ("ncomp", "int32_t", (), 8, 4), ("hmax", "int32_t", (), 12, 4),
          ("vmax", "int32_t", (), 16, 4), ("dri", "int32_t", (), 20, 4), ("n_intervals", "int32_t", (), 24, 4),
          ("reserved", "int32_t", (), 28, 4), ("tq", "uint8_t", (4,), 32, 4), ("td", "uint8_t", (4,), 36, 4), ("ta", "uint8_t", (4,), 40, 4),
          ("pad", "uint8_t", (4,), 44, 4), ("counts", "uint8_t", (4, 16), 48, 64), ("values", "uint8_t", (4, 256), 112, 1024),
          ("quant", "uint8_t", (4, 64), 1136, 256)]


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert hiplib.load().mi_abi_version() == 1
    assert [len(hiplib.SIGNATURES[n][1]) for n in NAMES] == [2, 2, 8, 7, 10, 7]
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for decl in ("int mi_jpeg_coefficients_device(int device, void* stream, const void* dev_span, size_t span_bytes, "
                 "const uint32_t* dev_offsets, const mi_jpeg_t* jpeg, int16_t* dev_coef, uint32_t* dev_status);",
                 "int mi_jpeg_coefficients(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, "
                 "const mi_jpeg_t* jpeg, int16_t* host_coef, uint32_t* status_out);",
                 "int mi_jpeg_decode_device(int device, void* stream, const void* dev_span, size_t span_bytes, "
                 "const uint32_t* dev_offsets, const mi_jpeg_t* jpeg, void* dev_scratch, size_t scratch_bytes, uint8_t* dev_out, "
                 "uint32_t* dev_status);",
                 "int mi_jpeg_decode(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, "
                 "const mi_jpeg_t* jpeg, uint8_t* host_out, uint32_t* status_out);"):
        assert decl in flat, decl
    assert re.search(r"#define MI_ABI_VERSION 1\b", text)
    for name, value in (("MI_JPEG_NOCODE", "1u"), ("MI_JPEG_OVERRUN", "2u"), ("MI_JPEG_RUN", "4u"), ("MI_JPEG_MAX_DRI", "8192")):
        assert re.search(r"#define %s %s\b" % (name, value), text), name
    from shinestacker_amd import jpeg
    assert (hiplib.JPEG_NOCODE, hiplib.JPEG_OVERRUN, hiplib.JPEG_RUN) == (1, 2, 4) and jpeg.MAX_DRI == 8192


def test_descriptor_layout(hiplib):
    text = open(HEADER).read()
    body = text[text.index("typedef struct mi_jpeg {"):text.index("} mi_jpeg_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    declared = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.match(r"(\w+)\s+(.+)$", decl.strip())
            for item in m.group(2).split(","):
                mm = re.match(r"(\w+)((?:\[\d+\])*)$", item.strip())
                declared.append((mm.group(1), m.group(1), tuple(int(d) for d in re.findall(r"\[(\d+)\]", mm.group(2)))))
    assert declared == [(n, t, dims) for n, t, dims, _, _ in FIELDS]
    mine = hiplib.JpegStruct
    assert [f[0] for f in mine._fields_] == [s[0] for s in FIELDS]
    for n, _, _, off, size in FIELDS:
        assert (getattr(mine, n).offset, getattr(mine, n).size) == (off, size), n
    assert ctypes.sizeof(mine) == 1392


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

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    calls = (lambda s, n, f, d, o: lib.mi_jpeg_coefficients_device(0, None, s, n, f, d, o if o is None else cp, None),
             lambda s, n, f, d, o: lib.mi_jpeg_coefficients(0, s, n, f, d, o if o is None else cp, stp),
             lambda s, n, f, d, o: lib.mi_jpeg_decode_device(0, None, s, n, f, d, 256, 1 << 20, o, None),
             lambda s, n, f, d, o: lib.mi_jpeg_decode(0, s, n, f, d, o, stp))
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
        expect(call(sp, 64, fp, desc(dri=0), op), b"jpeg dri must be in [1, 8192] (got 0)")
        expect(call(sp, 64, fp, desc(dri=8193, n_intervals=1), op), b"jpeg dri must be in [1, 8192] (got 8193)")
        expect(call(sp, 64, fp, desc(n_intervals=3), op), b"jpeg n_intervals must be ceil(2 MCUs / dri 1) = 2 (got 3)")
        expect(call(sp, 64, fp, desc(dri=2), op), b"jpeg n_intervals must be ceil(2 MCUs / dri 2) = 1 (got 2)")
        expect(call(sp, 64, fp, desc(tq=4), op), b"jpeg tq[2] must be in [0, 3] (got 4)")
        expect(call(sp, 64, fp, desc(td=2), op), b"jpeg td[2] must be 0 or 1 (got 2)")
        expect(call(sp, 64, fp, desc(ta=3), op), b"jpeg ta[2] must be 0 or 1 (got 3)")
        expect(call(sp, 64, fp, desc(quant=(1, 9, 0)), op), b"jpeg quant[1][9] must be >= 1")
        expect(call(sp, 64, fp, desc(counts=(2, [3])), op), b"jpeg counts[2] overflow the code space at length 1")
        expect(call(sp, 64, fp, desc(counts=(3, [1, 3])), op), b"jpeg counts[3] overflow the code space at length 2")
        expect(call(sp, 64, fp, desc(counts=(1, [0])), op), b"jpeg counts[1] must sum to 1 .. 256 (got 0)")
        expect(call(sp, 64, fp, desc(counts=(2, [0] * 8 + [200, 57])), op), b"jpeg counts[2] must sum to 1 .. 256 (got 257)")
        expect(call(sp, 64, fp, desc(value=(0, 0, 16)), op), b"jpeg values[0][0] must be <= 15 in a DC table (got 16)")
    # the host forms see the offsets
    for call in (calls[1], calls[3]):
        bad = np.array([0, 10, 65], np.uint32)
        expect(call(sp, 64, bad.ctypes.data, desc(), op), b"offsets[2] = 65 lies outside the span of 64 bytes")
        bad = np.array([12, 10, 20], np.uint32)
        expect(call(sp, 64, bad.ctypes.data, desc(), op), b"offsets[1] = 10 lies in front of offsets[0] = 12")
    # the device forms want buffers their accesses can take
    dev = lib.mi_jpeg_coefficients_device
    expect(dev(0, None, sp + 1, 63, fp, desc(), cp, None), b"dev_span must be 4-byte aligned")
    expect(dev(0, None, sp, 64, fp + 2, desc(), cp, None), b"dev_offsets must be 4-byte aligned")
    expect(dev(0, None, sp, 64, fp, desc(), cp + 2, None), b"dev_coef must be 16-byte aligned")
    expect(dev(0, None, sp, 64, fp, desc(), cp, stp + 2), b"dev_status must be 4-byte aligned")
    dec = lib.mi_jpeg_decode_device
    expect(dec(0, None, sp, 64, fp, desc(), None, 1 << 20, op, None), b"null scratch")
    expect(dec(0, None, sp, 64, fp, desc(), 256, 1151, op, None), b"scratch_bytes must be >= 1152 (got 1151)")
    expect(dec(0, None, sp, 64, fp, desc(), 384, 1 << 20, op, None), b"dev_scratch must be 256-byte aligned")
    # the two sizes
    n = ctypes.c_size_t(7)
    expect(lib.mi_jpeg_coef_count(None, ctypes.byref(n)), b"null jpeg")
    expect(lib.mi_jpeg_coef_count(desc(), None), b"null count")
    expect(lib.mi_jpeg_scratch_bytes(desc(ncomp=4), ctypes.byref(n)), b"jpeg ncomp must be 1 or 3 (got 4)")
    expect(lib.mi_jpeg_scratch_bytes(desc(), None), b"null bytes")
    assert n.value == 7
    assert lib.mi_jpeg_coef_count(desc(), ctypes.byref(n)) == hiplib.MI_OK and n.value == 6 * 64
    assert lib.mi_jpeg_scratch_bytes(desc(), ctypes.byref(n)) == hiplib.MI_OK and n.value == 6 * 192
    assert lib.mi_jpeg_coef_count(desc(hmax=2, vmax=2, n_intervals=1), ctypes.byref(n)) == hiplib.MI_OK and n.value == (4 + 1 + 1) * 64
    assert not out.any() and not status.any() and not coef.any()
    if hiplib.device_count() == 0:      # a valid call gets as far as asking for a device
        rc = lib.mi_jpeg_decode(0, sp, 64, fp, desc(), op, stp)
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
