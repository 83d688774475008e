"""CPU: the linear-frame entry points of the C boundary are declared, exported and bound, mi_linear_t as the header declares it
equals its ctypes mirror, and every argument check returns MI_ERR_INVALID with the argument named before any device call."""
import ctypes
import re

import numpy as np

from shinestacker_amd import demosaic
from test_develop_abi import HEADER, header_struct

NAMES = ("mi_linear_develop_device", "mi_linear_develop", "mi_linear_span")


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert hiplib.load().mi_abi_version() == 1
    assert len(hiplib.SIGNATURES["mi_linear_develop_device"][1]) == 9 and len(hiplib.SIGNATURES["mi_linear_develop"][1]) == 9
    # the structures beside it keep their layout: mi_raw_layout_t carries no spp, mi_ljpeg_seg_t stays 96 bytes
    assert "spp" not in [n for n, _, _ in header_struct("mi_raw_layout")]
    assert ctypes.sizeof(hiplib.LjpegSeg) == 96 and ctypes.sizeof(hiplib.RawLayoutStruct) == 56


def test_linear_struct_layout(hiplib):
    ct = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32}
    fields = header_struct("mi_linear")
    assert fields == [("black", "int32_t", 3), ("gain_q", "uint32_t", 3), ("white", "int32_t", 1), ("spp", "int32_t", 1)]

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, ct[t] * k if k > 1 else ct[t]) for n, t, k in fields]
    mine = hiplib.LinearStruct
    assert [f[0] for f in mine._fields_] == [n for n, _, _ in fields]
    for n, _, _ in fields:
        assert getattr(mine, n).offset == getattr(FromHeader, n).offset, n
        assert getattr(mine, n).size == getattr(FromHeader, n).size, n
    assert ctypes.sizeof(mine) == ctypes.sizeof(FromHeader) == 32
    s = demosaic.Linear(black=(1, 2, 3), gains=(1.0, 2.0, 0.5), white=1000).struct(np.uint16)
    assert (list(s.black), list(s.gain_q), s.white, s.spp) == ([1, 2, 3], [4096, 8192, 2048], 1000, 3)
    s = demosaic.Linear(black=5, gains=2.0, spp=1).struct(np.uint8)
    assert (s.black[0], s.gain_q[0], s.white, s.spp) == (5, 8192, 255, 1)


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    U8, U16, F32 = hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32
    a = np.zeros((4, 6, 3), np.uint16)
    out = np.zeros((4, 6, 3), np.uint16)
    ap, op = a.ctypes.data, out.ctypes.data

    def i32(*v):
        return (ctypes.c_int32 * len(v))(*v)

    def lin(black=(0, 0, 0), gain_q=(4096, 4096, 4096), white=65535, spp=3):
        return ctypes.byref(hiplib.LinearStruct(i32(*black), (ctypes.c_uint32 * 3)(*gain_q), white, spp))

    def dev(flags=0, mq=(4096, 0, 0, 0, 4096, 0, 0, 0, 4096), tone_ptr=None):
        return ctypes.byref(hiplib.DevelopStruct(flags, i32(*mq), tone_ptr))

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    over = (4096, 0, 0, 0, 4096, 0, 16384, -8192, 8192)            # row 2: 32768
    for host in (True, False):
        def call(samples=ap, bgr=op, h=4, w=6, dtype=U16, linear=lin(), mq=None, dv=None):
            if host:
                return lib.mi_linear_develop(0, samples, bgr, h, w, dtype, linear, None if mq is None else i32(*mq), None)
            return lib.mi_linear_develop_device(0, None, samples, bgr, h, w, dtype, linear, dv)
        expect(call(samples=None), b"null samples")
        expect(call(bgr=None), b"null bgr")
        expect(call(h=0), b"height and width must be >= 1 for a linear frame")
        expect(call(w=0), b"height and width must be >= 1 for a linear frame")
        expect(call(h=65536, w=32768), b"height x width too large")
        expect(call(linear=None), b"null linear")
        expect(call(dtype=F32), b"dtype must be MI_U8 or MI_U16 for a linear frame")
        expect(call(linear=lin(spp=2)), b"linear spp must be 1 or 3 (got 2)")
        expect(call(linear=lin(spp=4)), b"linear spp must be 1 or 3 (got 4)")
        expect(call(linear=lin(black=(0, -1, 0))), b"linear black[1] must be >= 0")
        expect(call(linear=lin(gain_q=(4096, 4096, 65536))), b"linear gain_q[2] must be <= 65535")
        expect(call(linear=lin(white=0)), b"linear white must be in [1, 65535]")
        expect(call(dtype=U8, linear=lin(white=256)), b"linear white must be in [1, 255]")
    expect(lib.mi_linear_develop(0, ap, op, 4, 6, U16, lin(), i32(*over), None), b"matrix_q row 2")
    expect(lib.mi_linear_develop_device(0, None, ap, op, 4, 6, U16, lin(), dev(flags=2)), b"MI_DEVELOP_TONE is set and dev_tone is null")
    expect(lib.mi_linear_develop_device(0, None, ap, op, 4, 6, U16, lin(), dev(flags=4)), b"unknown develop flags 4")
    expect(lib.mi_linear_develop_device(0, None, ap, op, 4, 6, U16, lin(), dev(flags=1, mq=over)), b"matrix_q row 2")
    expect(lib.mi_linear_develop_device(0, None, ap + 1, op, 4, 6, U16, lin(), None), b"must be aligned to their samples")
    expect(lib.mi_linear_develop_device(0, None, ap, op + 1, 4, 6, U16, lin(), None), b"must be aligned to their samples")
    if hiplib.device_count() == 0:      # a null develop is "plain", not an error: the call then asks for a device
        rc = lib.mi_linear_develop_device(0, None, ap, op, 1, 1, U16, lin(spp=1), None)
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
    text = open(HEADER).read()
    assert re.search(r"MI_API int mi_linear_span\(int dtype\);", text)


# ------------------------------------------------------------------------------------------------ mi_ljpeg_seg3_t, mi_raw_ljpeg3*
def test_seg3_is_128_bytes_and_matches_its_numpy_record(hiplib):
    ct = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8}
    text = open(HEADER).read()
    body = text[text.index("typedef struct mi_ljpeg_seg3 {"):text.index("} mi_ljpeg_seg3_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(\w+)\s+(\w+)((?:\[\d+\])*)\s*$", decl)
        if m:
            t = ct[m.group(1)]
            for n in reversed(re.findall(r"\[(\d+)\]", m.group(3))):
                t = t * int(n)
            fields.append((m.group(2), t))

    class FromHeader(ctypes.Structure):
        _fields_ = fields
    assert ctypes.sizeof(FromHeader) == 128 == hiplib.LJPEG_SEG3_DTYPE.itemsize
    assert [n for n, _ in fields] == list(hiplib.LJPEG_SEG3_DTYPE.names)
    for n, _ in fields:
        assert getattr(FromHeader, n).offset == hiplib.LJPEG_SEG3_DTYPE.fields[n][1], n
    assert hiplib.LJPEG_SEG3_DTYPE["counts"].shape == (3, 16) and hiplib.LJPEG_SEG3_DTYPE["values"].shape == (3, 17)
    # the head is mi_ljpeg_seg_t's: the same names at the same offsets up to the tables
    for n in ("scan_off", "scan_bytes", "x", "y", "ncomp", "predictor", "precision", "reserved", "counts"):
        assert hiplib.LJPEG_SEG3_DTYPE.fields[n][1] == hiplib.LJPEG_SEG_DTYPE.fields[n][1], n
    assert hiplib.LJPEG_SEG_DTYPE.itemsize == 96
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in ("mi_raw_ljpeg3", "mi_raw_ljpeg3_device"):
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert len(hiplib.SIGNATURES["mi_raw_ljpeg3"][1]) == len(hiplib.SIGNATURES["mi_raw_ljpeg"][1])
    assert len(hiplib.SIGNATURES["mi_raw_ljpeg3_device"][1]) == len(hiplib.SIGNATURES["mi_raw_ljpeg_device"][1])


def test_ljpeg3_argument_checks_come_before_any_device_call(hiplib, tmp_path):
    import linear_cases as LC
    from shinestacker_amd import dng
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    c = LC.LJPEG3["14bit-strips-of-3-short-last"]
    c.write(str(tmp_path / "a.dng"))
    frame = dng.read(str(tmp_path / "a.dng"))
    lay = frame.layout
    span = np.array(frame.span)
    out = np.zeros((lay.height, lay.width), np.uint16)
    status = np.zeros(3, np.uint32)

    def host(segs=lay.segments, L=None, span_p=span.ctypes.data, nbytes=span.nbytes, out_p=out.ctypes.data):
        L = lay.struct() if L is None else L
        return lib.mi_raw_ljpeg3(0, span_p, nbytes, None if segs is None else segs.ctypes.data, ctypes.byref(L), None, out_p, status.ctypes.data)

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    def changed(**kw):
        s = lay.segments.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s

    expect(host(span_p=None), b"null span")
    expect(host(segs=None), b"null segs")
    expect(host(out_p=None), b"null output")
    expect(host(nbytes=0), b"span_bytes must be in [1, 2^32)")
    L = lay.struct()
    L.bits = 9
    expect(host(L=L), b"layout bits must be 8, 10, 12, 14 or 16")
    for nc in (1, 2, 4):
        expect(host(segs=changed(ncomp=nc)), b"segs[1].ncomp must be 3 (got %d)" % nc)
    expect(host(segs=changed(predictor=0)), b"segs[1].predictor must be in [1, 7] (got 0)")
    expect(host(segs=changed(predictor=8)), b"segs[1].predictor must be in [1, 7] (got 8)")
    expect(host(segs=changed(precision=15)), b"segs[1].precision must be in [2, layout bits = 14] (got 15)")
    expect(host(segs=changed(precision=1)), b"segs[1].precision must be in [2, layout bits = 14] (got 1)")
    expect(host(segs=changed(x=lay.seg_width)), b"segs[1]: a frame of 3 lines of 54 x 3 samples does not match its segment of 3 x 54")
    expect(host(segs=changed(y=2)), b"segs[1]: a frame of 2 lines of 18 x 3 samples does not match its segment of 3 x 54")
    s = lay.segments.copy()
    s["counts"][1][2][:] = 0
    s["counts"][1][2][0] = 3
    expect(host(segs=s), b"segs[1].counts[2] overflow the code space at length 1")
    s = lay.segments.copy()
    s["counts"][1][0][:] = 0
    expect(host(segs=s), b"segs[1].counts[0] must sum to 1 .. 17 (got 0)")
    s = lay.segments.copy()
    s["values"][1][1][0] = 17
    expect(host(segs=s), b"segs[1].values[1][0] must be <= 16 (got 17)")
    expect(host(segs=changed(scan_bytes=span.nbytes)), b"outside the span of")
    wide = lay.struct()
    wide.image_width = wide.seg_width = wide.width = hiplib.LJPEG_MAX_LINE + 3
    s = lay.segments.copy()
    s["x"][:] = (hiplib.LJPEG_MAX_LINE + 3) // 3
    expect(host(segs=s, L=wide), b"segs[0].predictor 2 keeps the line above: layout seg_width must be <= 24576")
    # the device form: alignment
    L = lay.struct()
    p = span.ctypes.data
    sp = lay.segments.ctypes.data

    def devf(span_p=p & ~15, segs_p=sp & ~15, out_p=out.ctypes.data, st_p=status.ctypes.data):
        return lib.mi_raw_ljpeg3_device(0, None, span_p, span.nbytes, segs_p, ctypes.byref(L), None, out_p, st_p)
    expect(devf(span_p=None), b"null span")
    expect(devf(segs_p=None), b"null segs")
    expect(devf(span_p=(p & ~15) + 2), b"dev_span must be 4-byte aligned")
    expect(devf(segs_p=(sp & ~15) + 8), b"dev_segs must be 16-byte aligned")
    expect(devf(out_p=out.ctypes.data + 1), b"dev_out must be aligned to its samples")
    expect(devf(st_p=status.ctypes.data + 2), b"dev_status must be 4-byte aligned")


def test_push_linear_is_declared_exported_bound_and_checks_its_handle(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in ("mi_stack_push_linear", "mi_ljpeg3_batch"):
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert len(hiplib.SIGNATURES["mi_stack_push_linear"][1]) == 10
    lib = hiplib.load()
    span = np.zeros(16, np.uint8)
    offs = np.zeros(1, np.uint32)
    L = hiplib.RawLayoutStruct(8, 0, 2, 6, 0, 2, 6, 0, 0, 2, 6, 0, 0, hiplib.MI_U8)
    lin = demosaic.Linear().struct(np.uint8)
    rc = lib.mi_stack_push_linear(None, span.ctypes.data, span.nbytes, offs.ctypes.data, 0, ctypes.byref(L), None, ctypes.byref(lin), None, 0)
    assert rc == hiplib.MI_ERR_INVALID and b"null handle" in lib.mi_last_error()
    assert lib.mi_ljpeg3_batch() == hiplib.ljpeg3_batch() == 192 and hiplib.ljpeg3_batch() % 3 == 0
