"""CPU: the calibration entry points of the C boundary are declared, exported and bound, mi_calib_t as the header declares it
equals its ctypes mirror, and every argument check returns MI_ERR_INVALID with the argument named before any device call."""
import ctypes
import re

import numpy as np

from shinestacker_amd import Cfa
from test_develop_abi import HEADER, header_struct

NAMES = ("mi_mosaic_master_device", "mi_mosaic_master", "mi_flat_gain_device", "mi_flat_gain", "mi_mosaic_calibrate_device",
         "mi_mosaic_calibrate", "mi_stack_push_mosaic_calibrated")


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    text = open(HEADER).read()
    assert re.search(r"MI_CALIB_DARK = 1\b", text) and re.search(r"MI_CALIB_FLAT = 2\b", text)
    assert (hiplib.MI_CALIB_DARK, hiplib.MI_CALIB_FLAT) == (1, 2)
    assert hiplib.load().mi_abi_version() == 1
    nargs = {"mi_mosaic_master_device": 9, "mi_mosaic_master": 8, "mi_flat_gain_device": 9, "mi_flat_gain": 8,
             "mi_mosaic_calibrate_device": 8, "mi_mosaic_calibrate": 9, "mi_stack_push_mosaic_calibrated": 9}
    for name, n in nargs.items():
        assert len(hiplib.SIGNATURES[name][1]) == n, name
    # the entry points of the last releases keep their signatures
    C = ctypes
    cfa, dev = C.POINTER(hiplib.CfaStruct), C.POINTER(hiplib.DevelopStruct)
    assert hiplib.SIGNATURES["mi_stack_push_mosaic"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, cfa, C.c_int])
    assert hiplib.SIGNATURES["mi_stack_push_mosaic_developed"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, cfa, dev, C.c_void_p,
                                                                              C.c_int, C.c_int])
    assert hiplib.SIGNATURES["mi_demosaic"] == (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, cfa])
    assert hiplib.SIGNATURES["mi_develop"] == (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, cfa, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_int])
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for decl in ("int mi_stack_push_mosaic(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa, int pinned);",
                 "int mi_stack_push_mosaic_developed(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa, "
                 "const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned);",
                 "int mi_demosaic(int device, const void* host_mosaic, void* host_bgr, int height, int width, int dtype, const mi_cfa_t* cfa);",
                 "int mi_develop(int device, const void* host_mosaic, void* host_bgr, int height, int width, int dtype, const mi_cfa_t* cfa, "
                 "const int32_t* matrix_q, const void* host_tone, const int32_t* host_sites, int n);"):
        assert decl in flat, decl


def test_calib_struct_layout(hiplib):
    ct = {"int32_t": ctypes.c_int32, "const void*": ctypes.c_void_p, "const uint16_t*": ctypes.c_void_p}
    fields = header_struct("mi_calib")
    assert fields == [("flags", "int32_t", 1), ("dev_dark", "const void*", 1), ("dev_gain", "const uint16_t*", 1)]

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, ct[t] * k if k > 1 else ct[t]) for n, t, k in fields]
    mine = hiplib.CalibStruct
    assert [f[0] for f in mine._fields_] == [n for n, _, _ in fields]
    for n, _, _ in fields:
        assert getattr(mine, n).offset == getattr(FromHeader, n).offset, n
        assert getattr(mine, n).size == getattr(FromHeader, n).size, n
    assert ctypes.sizeof(mine) == ctypes.sizeof(FromHeader) == 24
    assert (mine.flags.offset, mine.dev_dark.offset, mine.dev_gain.offset) == (0, 8, 16)
    # mi_cfa_t and mi_develop_t are untouched
    assert header_struct("mi_cfa") == [("pattern", "int32_t", 1), ("black", "int32_t", 4), ("gain_q", "uint32_t", 4), ("white", "int32_t", 1)]
    assert header_struct("mi_develop") == [("flags", "int32_t", 1), ("matrix_q", "int32_t", 9), ("dev_tone", "const void*", 1)]
    assert ctypes.sizeof(hiplib.DevelopStruct) == 48 and ctypes.sizeof(hiplib.CfaStruct) == 40


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    U8, U16, F32 = hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32
    m = np.zeros((4, 6), np.uint16)
    out = np.zeros((4, 6), np.uint16)
    gain = np.full((4, 6), 16384, np.uint16)
    mp, op, gp = m.ctypes.data, out.ctypes.data, gain.ctypes.data
    cfa = ctypes.byref(Cfa().struct(np.uint16))
    bad_cfa = Cfa().struct(np.uint16)
    bad_cfa.black[2] = -1
    bad_cfa = ctypes.byref(bad_cfa)

    def cal(flags=0, dark=None, g=None):
        return ctypes.byref(hiplib.CalibStruct(flags, dark, g))

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*v)

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    # ---- mi_mosaic_master_device
    expect(lib.mi_mosaic_master_device(0, None, None, 3, 4, 6, U16, 1, op), b"null frames")
    expect(lib.mi_mosaic_master_device(0, None, mp, 3, 4, 6, U16, 1, None), b"null master output")
    expect(lib.mi_mosaic_master_device(0, None, mp, 3, 1, 6, U16, 1, op), b"height and width must be >= 2")
    expect(lib.mi_mosaic_master_device(0, None, mp, 3, 4, 1, U16, 1, op), b"height and width must be >= 2")
    expect(lib.mi_mosaic_master_device(0, None, mp, 3, 4, 6, F32, 1, op), b"dtype must be MI_U8 or MI_U16")
    expect(lib.mi_mosaic_master_device(0, None, mp, 3, 65536, 32768, U8, 1, op), b"height x width too large")
    expect(lib.mi_mosaic_master_device(0, None, mp, 0, 4, 6, U16, 0, op), b"number of frames must be in [1, 32] (got 0)")
    expect(lib.mi_mosaic_master_device(0, None, mp, 33, 4, 6, U16, 0, op), b"number of frames must be in [1, 32] (got 33)")
    expect(lib.mi_mosaic_master_device(0, None, mp, -1, 4, 6, U16, 0, op), b"number of frames must be in [1, 32]")
    expect(lib.mi_mosaic_master_device(0, None, mp, 3, 4, 6, U16, -1, op), b"reject must be >= 0 with 2 * reject < n (got -1, n = 3)")
    expect(lib.mi_mosaic_master_device(0, None, mp, 4, 4, 6, U16, 2, op), b"reject must be >= 0 with 2 * reject < n (got 2, n = 4)")
    expect(lib.mi_mosaic_master_device(0, None, mp, 1, 4, 6, U16, 1, op), b"reject must be >= 0")
    expect(lib.mi_mosaic_master_device(0, None, mp, 32, 4, 6, U16, 16, op), b"reject must be >= 0")
    expect(lib.mi_mosaic_master_device(0, None, mp, 3, 4, 6, U16, 2 ** 30 + 1, op), b"reject must be >= 0")

    # ---- mi_mosaic_master (host form)
    expect(lib.mi_mosaic_master(0, None, 3, 4, 6, U16, 1, op), b"null frames")
    expect(lib.mi_mosaic_master(0, ptrs(mp, mp, mp), 3, 4, 6, U16, 1, None), b"null master output")
    expect(lib.mi_mosaic_master(0, ptrs(mp, None, mp), 3, 4, 6, U16, 1, op), b"null frames[1]")
    expect(lib.mi_mosaic_master(0, ptrs(mp, mp, mp), 3, 4, 1, U16, 1, op), b"height and width must be >= 2")
    expect(lib.mi_mosaic_master(0, ptrs(mp, mp, mp), 3, 4, 6, F32, 1, op), b"dtype must be MI_U8 or MI_U16")
    expect(lib.mi_mosaic_master(0, ptrs(mp), 0, 4, 6, U16, 0, op), b"number of frames must be in [1, 32] (got 0)")
    expect(lib.mi_mosaic_master(0, ptrs(mp), 33, 4, 6, U16, 0, op), b"number of frames must be in [1, 32] (got 33)")
    expect(lib.mi_mosaic_master(0, ptrs(mp, mp), 2, 4, 6, U16, 1, op), b"reject must be >= 0 with 2 * reject < n (got 1, n = 2)")

    # ---- mi_flat_gain_device / mi_flat_gain
    for call in (lambda *a: lib.mi_flat_gain_device(0, None, *a), lambda *a: lib.mi_flat_gain(0, *a)):
        expect(call(None, None, 4, 6, U16, cfa, gp), b"null flat")
        expect(call(mp, None, 4, 6, U16, cfa, None), b"null gain output")
        expect(call(mp, None, 4, 6, U16, None, gp), b"null cfa")
        expect(call(mp, None, 1, 6, U16, cfa, gp), b"height and width must be >= 2")
        expect(call(mp, mp, 4, 6, F32, cfa, gp), b"dtype must be MI_U8 or MI_U16")
        expect(call(mp, mp, 32768, 65536, U16, cfa, gp), b"height x width too large")
        expect(call(mp, mp, 4, 6, U16, bad_cfa, gp), b"cfa black[2] must be >= 0")

    # ---- mi_mosaic_calibrate_device
    expect(lib.mi_mosaic_calibrate_device(0, None, None, 4, 6, U16, cfa, cal()), b"null mosaic")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, None, cal()), b"null cfa")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, cfa, None), b"null calib")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 1, 6, U16, cfa, cal()), b"height and width must be >= 2")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, F32, cfa, cal()), b"dtype must be MI_U8 or MI_U16")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 65536, 32768, U16, cfa, cal()), b"height x width too large")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, cfa, cal(4, mp, gp)), b"unknown calib flags 4")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, cfa, cal(1, None, gp)), b"MI_CALIB_DARK is set and dev_dark is null")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, cfa, cal(2, mp, None)), b"MI_CALIB_FLAT is set and dev_gain is null")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, cfa, cal(3, mp, None)), b"MI_CALIB_FLAT is set and dev_gain is null")
    expect(lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, bad_cfa, cal(1, mp)), b"cfa black[2] must be >= 0")
    # no flag: nothing to do, no device call -- whatever the pointers hold
    assert lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, cfa, cal()) == hiplib.MI_OK
    assert lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U8, ctypes.byref(Cfa().struct(np.uint8)), cal(0, None, gp)) == hiplib.MI_OK
    assert not m.any()
    if hiplib.device_count() == 0:      # a valid call gets as far as asking for a device
        rc = lib.mi_mosaic_calibrate_device(0, None, mp, 4, 6, U16, cfa, cal(1, mp))
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()

    # ---- mi_mosaic_calibrate (host form)
    expect(lib.mi_mosaic_calibrate(0, None, op, 4, 6, U16, cfa, None, None), b"null mosaic")
    expect(lib.mi_mosaic_calibrate(0, mp, None, 4, 6, U16, cfa, None, None), b"null mosaic output")
    expect(lib.mi_mosaic_calibrate(0, mp, op, 4, 6, U16, None, mp, gp), b"null cfa")
    expect(lib.mi_mosaic_calibrate(0, mp, op, 4, 1, U16, cfa, mp, gp), b"height and width must be >= 2")
    expect(lib.mi_mosaic_calibrate(0, mp, op, 4, 6, F32, cfa, mp, gp), b"dtype must be MI_U8 or MI_U16")
    expect(lib.mi_mosaic_calibrate(0, mp, op, 65536, 32768, U16, cfa, mp, gp), b"height x width too large")

    # ---- mi_stack_push_mosaic_calibrated
    expect(lib.mi_stack_push_mosaic_calibrated(None, mp, 0, cfa, cal(), None, None, 0, 0), b"null handle")
