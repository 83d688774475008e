"""CPU: the finishing entry points of the C boundary (mi_mosaic_radial_gain*, mi_frame_finish*) are declared, exported and bound,
mi_radial_gain_t as the header declares it equals its ctypes mirror, and every argument check returns MI_ERR_INVALID with the
argument named before any device call."""
import ctypes
import re

import numpy as np

from shinestacker_amd import Cfa
from test_develop_abi import HEADER, header_struct

NAMES = {"mi_mosaic_radial_gain_device": 8, "mi_mosaic_radial_gain": 8, "mi_frame_finish_device": 12, "mi_frame_finish": 11}


def test_entry_points_are_declared_exported_and_bound(hiplib):
    from test_abi import header_symbols
    cdll = ctypes.CDLL(hiplib.LIB_PATH)
    for name, n in NAMES.items():
        assert name in header_symbols() and name in hiplib.SIGNATURES and hasattr(cdll, name), name
        assert len(hiplib.SIGNATURES[name][1]) == n, name
    text = open(HEADER).read()
    assert re.search(r"#define MI_ABI_VERSION 1\b", text) and hiplib.load().mi_abi_version() == 1
    assert re.search(r"#define MI_RADIAL_NODES 1025\b", text) and hiplib.RADIAL_NODES == 1025


def test_radial_gain_struct_layout(hiplib):
    fields = header_struct("mi_radial_gain")
    assert fields == [("cx2", "int32_t", 1), ("cy2", "int32_t", 1), ("table", "const uint16_t*", 1)]
    mine = hiplib.RadialGainStruct
    assert [f[0] for f in mine._fields_] == ["cx2", "cy2", "table"]
    assert (mine.cx2.offset, mine.cy2.offset, mine.table.offset, ctypes.sizeof(mine)) == (0, 4, 8, 16)


def test_argument_checks_come_before_any_device_call(hiplib):
    lib = hiplib.load()
    INVALID = hiplib.MI_ERR_INVALID
    U8, U16, F32 = hiplib.MI_U8, hiplib.MI_U16, hiplib.MI_F32
    H, W = 4, 6
    m, out = np.zeros((H, W), np.uint16), np.zeros((H, W), np.uint16)
    mp, op = m.ctypes.data, out.ctypes.data
    cfa_s = Cfa(black=100).struct(np.uint16)
    cfa = ctypes.byref(cfa_s)
    table = np.full(hiplib.RADIAL_NODES, 4096, np.uint16)
    keep = []

    def rg(cx2=5, cy2=3, tab=table):
        s = hiplib.RadialGainStruct(cx2, cy2, None if tab is None else tab.ctypes.data)
        keep.append(s)
        return ctypes.byref(s)

    def expect(rc, msg):
        assert rc == INVALID, (msg, rc, lib.mi_last_error())
        assert msg in lib.mi_last_error(), (msg, lib.mi_last_error())

    forms = (lambda mo, h, w, dt, c, g: lib.mi_mosaic_radial_gain_device(0, None, mo, h, w, dt, c, g),
             lambda mo, h, w, dt, c, g: lib.mi_mosaic_radial_gain(0, mo, op, h, w, dt, c, g))
    for call in forms:
        expect(call(None, H, W, U16, cfa, rg()), b"null mosaic")
        expect(call(mp, H, W, U16, None, rg()), b"null cfa")
        expect(call(mp, H, W, U16, cfa, None), b"null radial gain")
        expect(call(mp, H, W, U16, cfa, rg(tab=None)), b"radial gain: null table")
        expect(call(mp, 1, W, U16, cfa, rg()), b"height and width must be >= 2")
        expect(call(mp, H, 1, U16, cfa, rg()), b"height and width must be >= 2")
        expect(call(mp, H, W, F32, cfa, rg()), b"dtype must be MI_U8 or MI_U16")
        expect(call(mp, 65536, 32768, U16, cfa, rg()), b"height x width too large")
        hi = Cfa(black=300).struct(np.uint8)
        expect(call(mp, H, W, U8, ctypes.byref(hi), rg()), b"cfa black[0] must be <= 255 (got 300)")
        expect(call(mp, H, W, U16, cfa, rg(cx2=(1 << 24) + 1)), b"at most 2^24 in magnitude")
        expect(call(mp, H, W, U16, cfa, rg(cy2=-(1 << 24) - 1)), b"at most 2^24 in magnitude")
        # a centre 2^23 pixels away: the farthest corner lies 2^48 half pixels squared from it
        expect(call(mp, H, W, U16, cfa, rg(cx2=1 << 24)), b"half pixels squared from the centre")
    expect(lib.mi_mosaic_radial_gain(0, mp, None, H, W, U16, cfa, rg()), b"null mosaic output")

    f, g = np.zeros((H, W, 3), np.uint16), np.zeros((H, W, 3), np.uint16)
    fp, gp = f.ctypes.data, g.ctypes.data
    forms = (lambda *a: lib.mi_frame_finish_device(0, None, *a), lambda *a: lib.mi_frame_finish(0, *a))
    for call in forms:
        expect(call(None, gp, H, W, U16, 0, 0, H, W, 1), b"null source frame")
        expect(call(fp, None, H, W, U16, 0, 0, H, W, 1), b"null destination frame")
        expect(call(fp, fp, H, W, U16, 0, 0, H, W, 1), b"source and destination must be distinct")
        expect(call(fp, gp, 0, W, U16, 0, 0, H, W, 1), b"height and width must be >= 1")
        expect(call(fp, gp, 65536, 32768, U16, 0, 0, H, W, 1), b"height x width too large")
        expect(call(fp, gp, H, W, F32, 0, 0, H, W, 1), b"dtype must be MI_U8 or MI_U16")
        for crop in ((-1, 0, H, W), (0, -1, H, W), (0, 0, 0, W), (0, 0, H, 0), (1, 0, H, W), (0, 1, H, W), (0, 0, H + 1, W),
                     (2 ** 31 - 1, 0, 2, W)):
            expect(call(fp, gp, H, W, U16, *crop, 1), b"must be a rectangle inside the 4 x 6 frame")
        expect(call(fp, gp, H, W, U16, 0, 0, H, W, 0), b"orientation must be in [1, 8] (got 0)")
        expect(call(fp, gp, H, W, U16, 0, 0, H, W, 9), b"orientation must be in [1, 8] (got 9)")
    if hiplib.device_count() == 0:      # a valid call gets as far as asking for a device
        rc = lib.mi_frame_finish(0, fp, gp, H, W, U16, 0, 0, H, W, 6)
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
        rc = lib.mi_mosaic_radial_gain(0, mp, op, H, W, U16, cfa, rg())
        assert rc != hiplib.MI_OK and rc != INVALID, lib.mi_last_error()
