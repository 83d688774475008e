"""CPU: the site-correction entry points of the C boundary are declared, exported and bound, mi_site_correct_t and its parts as
the header declares them equal their ctypes mirrors, every argument check returns MI_ERR_INVALID with the argument named before
any device call, MI_ABI_VERSION is 1 and the push entry points keep their signatures."""
import ctypes
import re

import numpy as np

from shinestacker_amd import Cfa
from test_develop_abi import HEADER, header_struct

NAMES = ("mi_mosaic_site_correct_device", "mi_mosaic_site_correct", "mi_mosaic_defects_const_device", "mi_stack_set_site_correction")
CT = {"int32_t": ctypes.c_int32, "uint16_t": ctypes.c_uint16, "const uint16_t*": ctypes.c_void_p, "const int16_t*": ctypes.c_void_p,
      "const int32_t*": ctypes.c_void_p, "const mi_site_axis_t*": ctypes.c_void_p, "void*": ctypes.c_void_p}


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    text = open(HEADER).read()
    assert re.search(r"#define MI_ABI_VERSION 1\b", text) and hiplib.load().mi_abi_version() == 1
    assert re.search(r"MI_SITE_DELTA_H = 1, MI_SITE_DELTA_V = 2, MI_SITE_GAIN = 4, MI_SITE_BAD_LIST = 8, MI_SITE_BAD_CONST = 16\b", text)
    assert (hiplib.MI_SITE_DELTA_H, hiplib.MI_SITE_DELTA_V, hiplib.MI_SITE_GAIN, hiplib.MI_SITE_BAD_LIST, hiplib.MI_SITE_BAD_CONST) == (1, 2, 4, 8, 16)
    nargs = {"mi_mosaic_site_correct_device": 8, "mi_mosaic_site_correct": 8, "mi_mosaic_defects_const_device": 9, "mi_stack_set_site_correction": 2}
    for name, n in nargs.items():
        assert len(hiplib.SIGNATURES[name][1]) == n, name


def test_the_push_entry_points_keep_their_signatures(hiplib):
    C = ctypes
    cfa, dev, cal, lay = (C.POINTER(hiplib.CfaStruct), C.POINTER(hiplib.DevelopStruct), C.POINTER(hiplib.CalibStruct),
                          C.POINTER(hiplib.RawLayoutStruct))
    S = hiplib.SIGNATURES
    assert S["mi_stack_push_mosaic"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, cfa, C.c_int])
    assert S["mi_stack_push_mosaic_developed"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, cfa, dev, C.c_void_p, C.c_int, C.c_int])
    assert S["mi_stack_push_mosaic_calibrated"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, cfa, cal, dev, C.c_void_p, C.c_int, C.c_int])
    packed = (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, lay, C.c_void_p, cfa, cal, dev, C.c_void_p, C.c_int, C.c_int])
    assert S["mi_stack_push_packed"] == packed and S["mi_stack_push_ljpeg"] == packed
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    for decl in ("int mi_stack_push_mosaic(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa, int pinned);",
                 "int mi_stack_push_mosaic_calibrated(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa, "
                 "const mi_calib_t* calib, const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned);",
                 "int mi_stack_push_packed(mi_stack_t* s, const void* host_span, size_t span_bytes, const uint32_t* seg_offsets, "
                 "const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_cfa_t* cfa, const mi_calib_t* calib, "
                 "const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned);",
                 "int mi_stack_push_ljpeg(mi_stack_t* s, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs, "
                 "const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_cfa_t* cfa, const mi_calib_t* calib, "
                 "const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned);",
                 "int mi_stack_set_site_correction(mi_stack_t* s, const mi_site_correct_t* sc);"):
        assert decl in flat, decl
    # the structs of the last releases are untouched
    assert header_struct("mi_calib") == [("flags", "int32_t", 1), ("dev_dark", "const void*", 1), ("dev_gain", "const uint16_t*", 1)]
    assert header_struct("mi_cfa") == [("pattern", "int32_t", 1), ("black", "int32_t", 4), ("gain_q", "uint32_t", 4), ("white", "int32_t", 1)]


def _same(mine, fields, ct):
    class FromHeader(ctypes.Structure):
        _fields_ = [(n, ct[t] * k if k > 1 else ct[t]) for n, t, k in fields]
    assert [f[0] for f in mine._fields_] == [n for n, _, _ in fields]
    for n, _, _ in fields:
        assert getattr(mine, n).offset == getattr(FromHeader, n).offset, n
        assert getattr(mine, n).size == getattr(FromHeader, n).size, n
    assert ctypes.sizeof(mine) == ctypes.sizeof(FromHeader)


def test_site_correct_struct_layout(hiplib):
    axis = header_struct("mi_site_axis")
    assert axis == [("node", "uint16_t", 1), ("weight", "uint16_t", 1)]
    assert hiplib.SITE_AXIS_DTYPE.itemsize == 4 and hiplib.SITE_AXIS_DTYPE.names == ("node", "weight")
    assert [hiplib.SITE_AXIS_DTYPE.fields[n][1] for n in ("node", "weight")] == [0, 2]
    gain = header_struct("mi_site_gain")
    assert gain == [("nodes", "const uint16_t*", 1), ("row_axis", "const mi_site_axis_t*", 1), ("col_axis", "const mi_site_axis_t*", 1),
                    ("mv", "int32_t", 1), ("mh", "int32_t", 1)]
    _same(hiplib.SiteGainStruct, gain, CT)
    assert ctypes.sizeof(hiplib.SiteGainStruct) == 32
    sc = header_struct("mi_site_correct")
    assert sc == [("flags", "int32_t", 1), ("delta_h", "const int16_t*", 1), ("delta_v", "const int16_t*", 1), ("gain", "mi_site_gain_t", 4),
                  ("bad_sites", "const int32_t*", 1), ("n_bad", "int32_t", 1), ("bad_constant", "int32_t", 1), ("bad_phase_mask", "int32_t", 1),
                  ("dev_scratch", "void*", 1)]
    _same(hiplib.SiteCorrectStruct, sc, dict(CT, mi_site_gain_t=hiplib.SiteGainStruct))
    mine = hiplib.SiteCorrectStruct
    assert ctypes.sizeof(mine) == 184 and mine.dev_scratch.offset == 176
    assert (mine.flags.offset, mine.delta_h.offset, mine.delta_v.offset, mine.gain.offset, mine.bad_sites.offset, mine.n_bad.offset,
            mine.bad_constant.offset, mine.bad_phase_mask.offset) == (0, 8, 16, 24, 152, 160, 164, 168)


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    U8, U16, F32 = hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32
    H, W = 4, 6
    m = np.zeros((H, W), np.uint16)
    out = np.zeros((H, W), np.uint16)
    mp, op = m.ctypes.data, out.ctypes.data
    cfa_s = Cfa(black=100).struct(np.uint16)
    cfa = ctypes.byref(cfa_s)
    bad_cfa = Cfa().struct(np.uint16)
    bad_cfa.black[2] = -1
    dh, dv = np.zeros(W, np.int16), np.zeros(H, np.int16)
    nodes = np.full((2, 3), 4096, np.uint16)
    ra, ca = np.zeros(H, hiplib.SITE_AXIS_DTYPE), np.zeros(W, hiplib.SITE_AXIS_DTYPE)
    sites = np.array([1, 5, 9], np.int32)
    keep = []

    def sc(flags=0, dh_=None, dv_=None, gains=None, bad=None, n_bad=0, constant=0, mask=15, scratch=True):
        s = hiplib.SiteCorrectStruct()
        s.flags = flags
        s.dev_scratch = mp if scratch else None
        s.delta_h = None if dh_ is None else dh_.ctypes.data
        s.delta_v = None if dv_ is None else dv_.ctypes.data
        for p, g in (gains or {}).items():
            n_, r_, c_, mv, mh = g
            s.gain[p].nodes = None if n_ is None else n_.ctypes.data
            s.gain[p].row_axis = None if r_ is None else r_.ctypes.data
            s.gain[p].col_axis = None if c_ is None else c_.ctypes.data
            s.gain[p].mv, s.gain[p].mh = mv, mh
        s.bad_sites = None if bad is None else bad.ctypes.data
        s.n_bad, s.bad_constant, s.bad_phase_mask = n_bad, constant, mask
        keep.append(s)
        return ctypes.byref(s)

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    forms = (lambda mo, h, w, dt, c, s: lib.mi_mosaic_site_correct_device(0, None, mo, h, w, dt, c, s),
             lambda mo, h, w, dt, c, s: lib.mi_mosaic_site_correct(0, mo, op, h, w, dt, c, s))
    for call in forms:
        expect(call(None, H, W, U16, cfa, sc()), b"null mosaic")
        expect(call(mp, H, W, U16, None, sc()), b"null cfa")
        expect(call(mp, H, W, U16, cfa, None), b"null site correction")
        expect(call(mp, 1, W, U16, cfa, sc()), b"height and width must be >= 2")
        expect(call(mp, H, 1, U16, cfa, sc()), b"height and width must be >= 2")
        expect(call(mp, H, W, F32, cfa, sc()), b"dtype must be MI_U8 or MI_U16")
        expect(call(mp, 65536, 32768, U16, cfa, sc()), b"height x width too large")
        expect(call(mp, H, W, U16, ctypes.byref(bad_cfa), sc()), b"cfa black[2] must be >= 0")
        expect(call(mp, H, W, U16, cfa, sc(32)), b"unknown site correction flags 32")
        expect(call(mp, H, W, U16, cfa, sc(1)), b"MI_SITE_DELTA_H is set and delta_h is null")
        expect(call(mp, H, W, U16, cfa, sc(2, dh)), b"MI_SITE_DELTA_V is set and delta_v is null")
        expect(call(mp, H, W, U16, cfa, sc(4)), b"MI_SITE_GAIN is set and every gain[].nodes is null")
        expect(call(mp, H, W, U16, cfa, sc(4, gains={1: (nodes, None, ca, 2, 3)})), b"gain[1] has nodes and row_axis is null")
        expect(call(mp, H, W, U16, cfa, sc(4, gains={2: (nodes, ra, None, 2, 3)})), b"gain[2] has nodes and col_axis is null")
        expect(call(mp, H, W, U16, cfa, sc(4, gains={0: (nodes, ra, ca, 0, 3)})), b"gain[0].mv must be in [1, 4096] (got 0)")
        expect(call(mp, H, W, U16, cfa, sc(4, gains={0: (nodes, ra, ca, 4097, 3)})), b"gain[0].mv must be in [1, 4096] (got 4097)")
        expect(call(mp, H, W, U16, cfa, sc(4, gains={3: (nodes, ra, ca, 2, 0)})), b"gain[3].mh must be in [1, 4096] (got 0)")
        expect(call(mp, H, W, U16, cfa, sc(4, gains={3: (nodes, ra, ca, 2, 5000)})), b"gain[3].mh must be in [1, 4096] (got 5000)")
        expect(call(mp, H, W, U16, cfa, sc(8, bad=sites, n_bad=-1)), b"n_bad must be >= 0 (got -1)")
        expect(call(mp, H, W, U16, cfa, sc(8, n_bad=3)), b"MI_SITE_BAD_LIST is set and bad_sites is null")
        expect(call(mp, H, W, U16, cfa, sc(16, constant=-1)), b"bad_constant must be in [0, 65535] (got -1)")
        expect(call(mp, H, W, U8, ctypes.byref(Cfa().struct(np.uint8)), sc(16, constant=256)), b"bad_constant must be in [0, 255] (got 256)")
        expect(call(mp, H, W, U16, cfa, sc(16, mask=0)), b"bad_phase_mask must be in [1, 15] (got 0)")
        expect(call(mp, H, W, U16, cfa, sc(16, mask=16)), b"bad_phase_mask must be in [1, 15] (got 16)")
    expect(forms[0](mp, H, W, U16, cfa, sc(16, scratch=False)), b"MI_SITE_BAD_CONST is set and dev_scratch is null")
    # no flag: nothing to do, no device call -- whatever the pointers hold
    assert lib.mi_mosaic_site_correct_device(0, None, mp, H, W, U16, cfa, sc()) == hiplib.MI_OK
    assert not m.any()

    # ---- tables in host memory: the host form reads them
    def host(s, c=cfa, dt=U16):
        return lib.mi_mosaic_site_correct(0, mp, op, H, W, dt, c, s)
    w_bad, n_bad = ca.copy(), ra.copy()
    w_bad["weight"][3] = 257
    n_bad["node"][2] = 2
    expect(host(sc(4, gains={1: (nodes, ra, w_bad, 2, 3)})), b"gain[1].col_axis[3].weight must be <= 256 (got 257)")
    expect(host(sc(4, gains={0: (nodes, n_bad, ca, 2, 3)})), b"gain[0].row_axis[2].node = 2 lies outside the 2 rows of its grid")
    c_bad = ca.copy()
    c_bad["node"][4] = 3
    expect(host(sc(4, gains={2: (nodes, ra, c_bad, 2, 3)})), b"gain[2].col_axis[4].node = 3 lies outside the 3 columns of its grid")
    low, high = dh.copy(), dv.copy()
    low[1] = -101
    expect(host(sc(1, low)), b"black[1] + delta_h + delta_v must stay inside [0, 65535] (it spans -1 .. 100)")
    high[3] = 32767
    hi_cfa = Cfa(black=40000).struct(np.uint16)
    expect(host(sc(3, dh, high), ctypes.byref(hi_cfa)), b"black[2] + delta_h + delta_v must stay inside [0, 65535] (it spans 40000 .. 72767)")
    expect(host(sc(8, bad=np.array([1, 5, 5], np.int32), n_bad=3)), b"sites must be strictly ascending")
    expect(host(sc(8, bad=np.array([1, 5, 24], np.int32), n_bad=3)), b"sites[2] = 24 lies outside the 6 x 4 image")

    # ---- mi_mosaic_defects_const_device
    expect(lib.mi_mosaic_defects_const_device(0, None, None, H, W, U16, 5, 15, mp), b"null mosaic")
    expect(lib.mi_mosaic_defects_const_device(0, None, mp, 1, W, U16, 5, 15, mp), b"height and width must be >= 2")
    expect(lib.mi_mosaic_defects_const_device(0, None, mp, H, W, F32, 5, 15, mp), b"dtype must be MI_U8 or MI_U16")
    expect(lib.mi_mosaic_defects_const_device(0, None, mp, 32768, 65536, U16, 5, 15, mp), b"height x width too large")
    expect(lib.mi_mosaic_defects_const_device(0, None, mp, H, W, U8, 256, 15, mp), b"bad_constant must be in [0, 255]")
    expect(lib.mi_mosaic_defects_const_device(0, None, mp, H, W, U16, 5, 0, mp), b"bad_phase_mask must be in [1, 15]")
    expect(lib.mi_mosaic_defects_const_device(0, None, mp, H, W, U16, 5, 15, None), b"MI_SITE_BAD_CONST is set and dev_scratch is null")

    # ---- mi_stack_set_site_correction
    expect(lib.mi_stack_set_site_correction(None, sc()), b"null handle")
    if hiplib.device_count() == 0:      # a valid call gets as far as asking for a device
        rc = lib.mi_mosaic_site_correct(0, mp, op, H, W, U16, cfa, sc(3, dh, dv))
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
