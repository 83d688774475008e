"""CPU: the development entry points of the C boundary are declared, exported and bound, mi_develop_t as the header declares it
equals its ctypes mirror, and every argument check returns MI_ERR_INVALID with the argument named before any device call."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
from shinestacker_amd import Cfa

HEADER = os.path.join(ROOT, "include", "mi355stack.h")
NAMES = ("mi_mosaic_defects_device", "mi_develop_device", "mi_develop", "mi_stack_push_mosaic_developed")


def header_struct(name):
    """(member, ctype, count) of `typedef struct <name> { ... } <name>_t;`, parsed from the header"""
    text = open(HEADER).read()
    body = text[text.index("typedef struct %s {" % name):text.index("} %s_t;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(.+?)\s*(\w+)(?:\[(\d+)\])?$", decl)
        fields.append((m.group(2), m.group(1).strip(), int(m.group(3) or 1)))
    return fields


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
    text = open(HEADER).read()
    assert re.search(r"MI_DEVELOP_MATRIX = 1\b", text) and re.search(r"MI_DEVELOP_TONE = 2\b", text)
    assert (hiplib.MI_DEVELOP_MATRIX, hiplib.MI_DEVELOP_TONE) == (1, 2)
    assert hiplib.load().mi_abi_version() == 1
    # the entry points of the last release keep their signatures
    assert len(hiplib.SIGNATURES["mi_stack_push_mosaic"][1]) == 5 and len(hiplib.SIGNATURES["mi_demosaic"][1]) == 7


def test_develop_struct_layout(hiplib):
    ct = {"int32_t": ctypes.c_int32, "const void*": ctypes.c_void_p}
    fields = header_struct("mi_develop")
    assert fields == [("flags", "int32_t", 1), ("matrix_q", "int32_t", 9), ("dev_tone", "const void*", 1)]

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, ct[t] * k if k > 1 else ct[t]) for n, t, k in fields]
    mine = hiplib.DevelopStruct
    assert [f[0] for f in mine._fields_] == [n for n, _, _ in fields]
    for n, _, _ in fields:
        assert getattr(mine, n).offset == getattr(FromHeader, n).offset, n
        assert getattr(mine, n).size == getattr(FromHeader, n).size, n
    assert ctypes.sizeof(mine) == ctypes.sizeof(FromHeader) == 48
    assert (mine.flags.offset, mine.matrix_q.offset, mine.dev_tone.offset) == (0, 4, 40)
    # mi_cfa_t is untouched
    assert [(n, t, k) for n, t, k in header_struct("mi_cfa")] == [("pattern", "int32_t", 1), ("black", "int32_t", 4),
                                                                 ("gain_q", "uint32_t", 4), ("white", "int32_t", 1)]


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    U8, U16, F32 = hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32
    m = np.zeros((4, 6), np.uint16)
    out = np.zeros((4, 6, 3), np.uint16)
    tone = np.arange(65536).astype(np.uint16)
    mp, op, tp = m.ctypes.data, out.ctypes.data, tone.ctypes.data
    cfa = ctypes.byref(Cfa().struct(np.uint16))

    def i32(*v):
        return (ctypes.c_int32 * len(v))(*v)

    def dev(flags=0, mq=(4096, 0, 0, 0, 4096, 0, 0, 0, 4096), tone_ptr=None):
        return ctypes.byref(hiplib.DevelopStruct(flags, i32(*mq), tone_ptr))

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    ident = i32(4096, 0, 0, 0, 4096, 0, 0, 0, 4096)
    over = (4096, 0, 0, 0, 4096, 0, 16384, -8192, 8192)            # row 2: 32768
    at = (16384, -8192, -8191, 0, 4096, 0, 0, 0, 4096)             # row 0: 32767, inside the bound
    sites = i32(0, 5, 23)

    # ---- mi_develop (host form)
    expect(lib.mi_develop(0, None, op, 4, 6, U16, cfa, None, None, None, 0), b"null mosaic")
    expect(lib.mi_develop(0, mp, None, 4, 6, U16, cfa, None, None, None, 0), b"null bgr")
    expect(lib.mi_develop(0, mp, op, 4, 6, U16, None, None, None, None, 0), b"null cfa")
    expect(lib.mi_develop(0, mp, op, 1, 6, U16, cfa, None, None, None, 0), b"height and width must be >= 2")
    expect(lib.mi_develop(0, mp, op, 4, 6, F32, cfa, None, None, None, 0), b"dtype must be MI_U8 or MI_U16")
    expect(lib.mi_develop(0, mp, op, 4, 6, U16, cfa, i32(*over), None, None, 0), b"matrix_q row 2")
    assert b"32767" in lib.mi_last_error() and b"32768" in lib.mi_last_error()
    expect(lib.mi_develop(0, mp, op, 4, 6, U16, cfa, ident, tp, None, -1), b"number of sites must be >= 0")
    expect(lib.mi_develop(0, mp, op, 4, 6, U16, cfa, ident, tp, None, 3), b"null sites")
    expect(lib.mi_develop(0, mp, op, 4, 6, U16, cfa, None, None, i32(0, 5, 24), 3), b"sites[2] = 24 lies outside")
    expect(lib.mi_develop(0, mp, op, 4, 6, U16, cfa, None, None, i32(-1, 5, 23), 3), b"sites[0] = -1 lies outside")
    expect(lib.mi_develop(0, mp, op, 4, 6, U16, cfa, None, None, i32(0, 5, 5), 3), b"sites must be strictly ascending (sites[2]")
    expect(lib.mi_develop(0, mp, op, 4, 6, U16, cfa, None, None, i32(7, 5, 9), 3), b"sites must be strictly ascending (sites[1]")

    # ---- mi_develop_device
    expect(lib.mi_develop_device(0, None, None, op, 4, 6, U16, cfa, dev()), b"null mosaic")
    expect(lib.mi_develop_device(0, None, mp, None, 4, 6, U16, cfa, dev()), b"null bgr")
    expect(lib.mi_develop_device(0, None, mp, op, 4, 6, U16, None, dev()), b"null cfa")
    expect(lib.mi_develop_device(0, None, mp, op, 4, 6, U16, cfa, None), b"null develop")
    expect(lib.mi_develop_device(0, None, mp, op, 4, 6, U16, cfa, dev(flags=2)), b"MI_DEVELOP_TONE is set and dev_tone is null")
    expect(lib.mi_develop_device(0, None, mp, op, 4, 6, U16, cfa, dev(flags=3)), b"MI_DEVELOP_TONE is set and dev_tone is null")
    expect(lib.mi_develop_device(0, None, mp, op, 4, 6, U16, cfa, dev(flags=4)), b"unknown develop flags 4")
    expect(lib.mi_develop_device(0, None, mp, op, 4, 6, U16, cfa, dev(flags=1, mq=over)), b"matrix_q row 2")
    expect(lib.mi_develop_device(0, None, mp, op, 4, 6, F32, cfa, dev(flags=1)), b"dtype must be MI_U8 or MI_U16")
    # the matrix is only read under its flag; a row AT the bound passes the check (the call then asks for a device)
    assert lib.mi_develop_device(0, None, mp, op, 4, 6, F32, cfa, dev(flags=0, mq=over)) == INVALID and b"dtype" in lib.mi_last_error()
    if hiplib.device_count() == 0:
        rc = lib.mi_develop_device(0, None, mp, op, 4, 6, U16, cfa, dev(flags=1, mq=at))
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()

    # ---- mi_mosaic_defects_device
    expect(lib.mi_mosaic_defects_device(0, None, None, 4, 6, U16, sites, 3), b"null mosaic")
    expect(lib.mi_mosaic_defects_device(0, None, mp, 4, 1, U16, sites, 3), b"height and width must be >= 2")
    expect(lib.mi_mosaic_defects_device(0, None, mp, 4, 6, F32, sites, 3), b"dtype must be MI_U8 or MI_U16")
    expect(lib.mi_mosaic_defects_device(0, None, mp, 4, 6, U16, sites, -1), b"number of sites must be >= 0")
    expect(lib.mi_mosaic_defects_device(0, None, mp, 4, 6, U16, None, 3), b"null sites")
    expect(lib.mi_mosaic_defects_device(0, None, mp, 65536, 32768, U8, sites, 3), b"height x width too large")
    assert lib.mi_mosaic_defects_device(0, None, mp, 4, 6, U16, None, 0) == hiplib.MI_OK       # nothing to do, no device call

    # ---- mi_stack_push_mosaic_developed
    expect(lib.mi_stack_push_mosaic_developed(None, mp, 0, cfa, dev(), None, 0, 0), b"null handle")
