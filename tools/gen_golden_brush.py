#!/usr/bin/env python3
"""Record tests/golden/brush.npz + brush.json from the reference's OWN retouch/brush_preview.py, retouch/brush_tool.py and
retouch/undo_manager.py.

    python tools/gen_golden_brush.py          (needs the reference tree; see oracle/ref_import.py)

The three modules import PySide6, which is not installed here and is not needed for their arithmetic: stand-in `PySide6`
modules are defined below (every Qt class is an empty class, a Signal emits into nothing).  The parent packages are seeded as
empty modules whose __path__ points at the real directories, so no package __init__ runs.  Inside brush_preview the name
`np` is a proxy that is NumPy except for `cos` and `power` on float64, which go through long double and are rounded once --
NumPy's float64 SIMD transcendentals depend on the CPU; oracle/ref_import.py does the same for log and exp.

A stroke is driven the way retouch/image_editor_ui.py:511-539 drives it: a zero float64 mask layer and a copy of the master at
the start, then for every stamp `BrushTool.apply_brush_operation(master copy, source, master, mask layer, position)` and
`UndoManager.extend_undo_area(*area)`; the viewer's mapToScene is the identity on float positions.  Data only: frames, brushes,
stamp positions, the tables, the painted frames, the mask layers and the undo areas.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BRUSHES = [(5, 50, 100, 100), (13, 0, 70, 30), (21, 100, 100, 50), (9.7, 85, 55, 100), (30, 20, 100, 7)]   # size, hardness, opacity, flow


class _QtClass:
    """stand-in for every Qt class: constructible, subclassable, every method does nothing"""

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return lambda *a, **k: None


class _Signal:
    def __init__(self, *a):
        pass

    def emit(self, *a):
        pass

    def connect(self, *a):
        pass


class _QtModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Signal if name == "Signal" else _QtClass


class _NumpyWithLongDoubleProfile:
    """`np` inside brush_preview: float64 cos and power through long double, rounded once"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def cos(x):
        x = np.asarray(x)
        return np.cos(x.astype(np.longdouble)).astype(np.float64) if x.dtype == np.float64 else np.cos(x)

    @staticmethod
    def power(x, k):
        x = np.asarray(x)
        return np.power(x.astype(np.longdouble), np.longdouble(k)).astype(np.float64) if x.dtype == np.float64 else np.power(x, k)


def load_reference():
    if not ref_import.available():
        raise SystemExit("reference tree not present")
    sys.dont_write_bytecode = True
    for name in [m for m in sys.modules if m.startswith(("shinestacker", "PySide6"))]:
        del sys.modules[name]
    for pkg in ("shinestacker", "shinestacker.retouch", "shinestacker.config"):
        mod = types.ModuleType(pkg)
        mod.__path__ = [os.path.join(ref_import.REF_SRC, *pkg.split("."))]
        sys.modules[pkg] = mod
    for name in ("PySide6", "PySide6.QtWidgets", "PySide6.QtGui", "PySide6.QtCore"):
        sys.modules[name] = _QtModule(name)
    mods = [importlib.import_module("shinestacker.retouch." + m) for m in ("brush_preview", "brush_tool", "undo_manager")]
    assert all(m.__file__.startswith(ref_import.REF_SRC) for m in mods)
    return mods


class _Pos:
    def __init__(self, x, y):
        self._x, self._y = x, y

    def x(self):
        return self._x

    def y(self):
        return self._y


class _Viewer:
    @staticmethod
    def mapToScene(pos):
        return pos


def paint(bt, um, master, source, brush, points):
    """one stroke as the editor runs it: (frame, mask layer, area, table)"""
    tool = bt.BrushTool()
    tool.brush = types.SimpleNamespace(size=brush[0], hardness=brush[1], opacity=brush[2], flow=brush[3])
    tool.image_viewer = _Viewer()
    undo = um.UndoManager()
    mask_layer = np.zeros(master.shape[:2])
    kept, dest = master.copy(), master.copy()
    undo.reset_undo_area()
    for x, y in points:
        undo.extend_undo_area(*tool.apply_brush_operation(kept, source, dest, mask_layer, _Pos(x, y)))
    area = (undo.x_start, undo.y_start, undo.x_end, undo.y_end)
    if not (area[2] > 0 and area[3] > 0):
        area = (0, 0, 0, 0)
    radius = int(round(brush[0] // 2))
    return dest, mask_layer, [int(v) for v in area], tool.get_brush_mask(radius)


def lowbias32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def synth(h, w, seed, dtype):
    """A smooth texture that spans the type's range plus integer hash noise in [-2, 2]; the uint16 frame is the uint8 one
    widened with a low byte derived from it.  The texture is rounded from float64 sines once, here: the frames are recorded, not rebuilt."""
    y, x = np.mgrid[:h, :w]
    tex = 128.0 + 120.0 * np.sin(x / (4.0 + seed)) * np.cos(y / (3.0 + seed))
    idx = np.arange(h * w * 3, dtype=np.uint32).reshape(h, w, 3) + np.uint32(seed * 7919)
    noise = (lowbias32(idx) % np.uint32(5)).astype(np.int64) - 2
    a = np.clip(np.rint(tex).astype(np.int64)[:, :, None] + np.array([5, 0, -4]) * seed + noise, 0, 255).astype(np.uint32)
    if np.dtype(dtype) == np.uint8:
        return a.astype(np.uint8)
    return ((a << 8) | ((a * 37 + 11) & 255)).astype(np.uint16)


def edge_stamps(h, w):
    """34 positions: inside, half-way coordinates, clipped at every edge and corner, and outside on every side"""
    inside = [(10, 8), (11.5, 8.5), (12.5, 9.5), (13, 10), (14.2, 10.7), (14.2, 10.7), (20, 20), (21, 20), (22, 21), (26.49, 18.51),
              (30, 15), (31, 15), (32, 15), (33, 16)]
    clipped = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w / 2, 0), (w / 2, h - 1), (0, h / 2), (w - 1, h / 2), (-2, 5), (w + 1, 7),
               (9, -2), (17, h + 1)]
    outside = [(-40, 10), (w + 40, 10), (10, -40), (10, h + 40), (-100, -100), (w + 16, h + 16), (1e6, 3), (3, -1e6)]
    return inside + clipped + outside


def main():
    bp, bt, um = load_reference()
    plain = {b: bp.create_brush_mask(2 * int(round(b[0] // 2)) + 1, b[1], b[2]) for b in BRUSHES}
    bp.np = _NumpyWithLongDoubleProfile()
    arrays, cases = {}, []
    frames = {}
    for name, (h, w) in (("odd", (37, 53)),):
        for dt in (np.uint8, np.uint16):
            key = f"{name}_{np.dtype(dt).name}"
            frames[key] = (synth(h, w, 1, dt), synth(h, w, 2, dt))
            arrays[f"master_{key}"], arrays[f"source_{key}"] = frames[key]

    stamp_lists = {}

    def record(name, frame, brush, points, pkey=None):
        pkey = pkey or name.rsplit("_", 1)[0]
        stamp_lists.setdefault(pkey, [[float(x), float(y)] for x, y in points])
        master, source = frames[frame]
        out, layer, area, table = paint(bt, um, master, source, brush, points)
        assert out.dtype == master.dtype and layer.dtype == np.float64 and table.dtype == np.float64
        tkey = "table_" + "_".join(str(v) for v in (2 * int(round(brush[0] // 2)) + 1, brush[1], brush[2]))
        if tkey in arrays:
            assert np.array_equal(arrays[tkey], table)
        arrays[tkey] = table
        lkey = "layer_" + name.rsplit("_", 1)[0]       # the mask layer does not depend on the frames: one per stroke
        if lkey in arrays:
            assert np.array_equal(arrays[lkey], layer)
        okey = f"out_{name}"
        if np.array_equal(out, master):             # nothing was painted: the expected frame is the master, stored once
            okey = f"master_{frame}"
        else:
            arrays[okey] = out
        arrays[lkey] = layer
        cases.append({"name": name, "frame": frame, "brush": list(brush), "points": pkey,
                      "table": tkey, "layer": lkey, "out": okey, "area": area, "changed_values": int((out != master).sum()),
                      "saturated_mask": int((layer == 1.0).sum())})

    for i, b in enumerate(BRUSHES):             # the five brushes over the 34 stamps, both depths
        for dt in ("uint8", "uint16"):
            record(f"b{i}_{dt}", f"odd_{dt}", b, edge_stamps(37, 53), "edges")
    record("miss_uint8", "odd_uint8", BRUSHES[0], [(-40, 10), (200, 10), (10, -40), (10, 300)])       # every stamp misses the frame
    record("empty_uint16", "odd_uint16", BRUSHES[1], [])
    record("single_uint8", "odd_uint8", BRUSHES[2], [(31.5, 24.5)])
    record("repeat_uint16", "odd_uint16", BRUSHES[4], [(20 + 0.5 * k, 24) for k in range(40)])      # flow 7: order-dependent sums
    record("inside_uint8", "odd_uint8", BRUSHES[3], [(20, 20), (40, 30), (41, 30)])             # no miss: the area is tight

    differs = {"_".join(str(v) for v in b): int((plain[b] != arrays["table_" + "_".join(
        str(v) for v in (2 * int(round(b[0] // 2)) + 1, b[1], b[2]))]).sum()) for b in BRUSHES}
    meta = {"cases": cases, "stamp_lists": stamp_lists, "brushes": [list(b) for b in BRUSHES],
            "table_entries_where_plain_numpy_differs_on_the_recording_box": differs}
    np.savez_compressed(os.path.join(GOLDEN, "brush.npz"), **arrays)
    with open(os.path.join(GOLDEN, "brush.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote brush.npz", os.path.getsize(os.path.join(GOLDEN, "brush.npz")), "bytes, brush.json",
          os.path.getsize(os.path.join(GOLDEN, "brush.json")), "bytes;", len(cases), "cases")
    for c in cases:
        print(" ", c["name"], "area", c["area"], "changed", c["changed_values"], "saturated", c["saturated_mask"])
    print("  plain NumPy differs:", differs)


if __name__ == "__main__":
    main()
