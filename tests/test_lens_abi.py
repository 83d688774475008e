"""CPU: the lens entry points of the C boundary are declared, exported and bound, mi_lens_t as the header declares it equals its
ctypes mirror, and every argument check returns MI_ERR_INVALID with the argument named before any device call."""
import ctypes
import re

import numpy as np

from test_develop_abi import HEADER, header_struct

NAMES = ("mi_lens_remap_device", "mi_lens_remap")


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    assert hiplib.load().mi_abi_version() == 1
    C = ctypes
    lens = C.POINTER(hiplib.LensStruct)
    assert hiplib.SIGNATURES["mi_lens_remap_device"] == (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                                  C.c_int, C.c_int, lens])
    assert hiplib.SIGNATURES["mi_lens_remap"] == (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, lens])
    assert [len(hiplib.SIGNATURES[n][1]) for n in NAMES] == [9, 8]
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    for decl in ("int mi_lens_remap_device(int device, void* stream, const void* dev_src, void* dev_dst, void* dev_mask, int height, "
                 "int width, int dtype, const mi_lens_t* lens);",
                 "int mi_lens_remap(int device, const void* host_src, void* host_dst, void* host_mask, int height, int width, int dtype, "
                 "const mi_lens_t* lens);"):
        assert decl in flat, decl
    assert re.search(r"#define MI_ABI_VERSION 1\b", open(HEADER).read())


def test_lens_struct_layout(hiplib):
    fields = header_struct("mi_lens")
    assert fields == [("k", "double", 12), ("cx", "double", 1), ("cy", "double", 1)]

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, ctypes.c_double * k if k > 1 else ctypes.c_double) for n, _, k in fields]
    mine = hiplib.LensStruct
    assert [f[0] for f in mine._fields_] == [n for n, _, _ in fields]
    for n, _, _ in fields:
        assert getattr(mine, n).offset == getattr(FromHeader, n).offset, n
        assert getattr(mine, n).size == getattr(FromHeader, n).size, n
    assert ctypes.sizeof(mine) == ctypes.sizeof(FromHeader) == 112
    assert (mine.k.offset, mine.cx.offset, mine.cy.offset) == (0, 96, 104)


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    U8, U16, F32 = hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32
    src, dst = np.zeros((4, 6, 3), np.uint16), np.zeros((4, 6, 3), np.uint16)
    mask = np.zeros((4, 6), np.uint8)
    sp, dp, mp = src.ctypes.data, dst.ctypes.data, mask.ctypes.data

    def lens(**bad):
        s = hiplib.LensStruct((ctypes.c_double * 12)(*([1, 0, 0, 0] * 3)), 2.5, 1.5)
        for name, v in bad.items():
            if name.startswith("k"):
                s.k[int(name[1:])] = v
            else:
                setattr(s, name, v)
        return ctypes.byref(s)

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    nan, inf = float("nan"), float("inf")
    for call in (lambda s, d, m, *a: lib.mi_lens_remap_device(0, None, s, d, m, *a), lambda s, d, m, *a: lib.mi_lens_remap(0, s, d, m, *a)):
        expect(call(None, dp, mp, 4, 6, U16, lens()), b"null source frame")
        expect(call(sp, None, mp, 4, 6, U16, lens()), b"null destination frame")
        expect(call(sp, dp, mp, 4, 6, U16, None), b"null lens")
        expect(call(sp, sp, None, 4, 6, U16, lens()), b"source and destination must be distinct")
        expect(call(sp, dp, None, 0, 6, U16, lens()), b"height and width must be >= 1")
        expect(call(sp, dp, None, 4, 0, U16, lens()), b"height and width must be >= 1")
        expect(call(sp, dp, None, -4, 6, U16, lens()), b"height and width must be >= 1")
        expect(call(sp, dp, None, 65536, 32768, U8, lens()), b"height x width too large")
        expect(call(sp, dp, None, 1, 1 << 26, U8, lens()), b"height x width too large")
        expect(call(sp, dp, None, 1 << 26, 2, U16, lens()), b"height x width too large")
        expect(call(sp, dp, None, 4, 6, F32, lens()), b"dtype must be MI_U8 or MI_U16")
        expect(call(sp, dp, None, 4, 6, 7, lens()), b"dtype must be MI_U8 or MI_U16")
        expect(call(sp, dp, None, 4, 6, U16, lens(k0=nan)), b"lens k[0] must be finite")
        expect(call(sp, dp, None, 4, 6, U16, lens(k5=inf)), b"lens k[5] must be finite")
        expect(call(sp, dp, mp, 4, 6, U8, lens(k11=-inf)), b"lens k[11] must be finite")
        expect(call(sp, dp, None, 4, 6, U16, lens(cx=nan)), b"lens cx must be finite")
        expect(call(sp, dp, None, 4, 6, U16, lens(cy=-inf)), b"lens cy must be finite")
        expect(call(sp, dp, None, 4, 6, U16, lens(cx=2.0 ** 30 + 1)), b"lens cx must be finite and at most 2^30 in magnitude")
        expect(call(sp, dp, None, 4, 6, U16, lens(cy=-1e300)), b"lens cy must be finite and at most 2^30 in magnitude")
    assert not dst.any() and not mask.any()
    if hiplib.device_count() == 0:      # a valid call gets as far as asking for a device
        rc = lib.mi_lens_remap(0, sp, dp, None, 4, 6, U16, lens())
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
