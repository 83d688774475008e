#!/usr/bin/env python3
"""Record tests/golden/retouch.npz + retouch.json from the reference's OWN sharpen.py and white_balance.py.

    python tools/gen_golden_retouch.py          (needs the reference tree; see oracle/ref_import.py)

The reference's algorithms/sharpen.py and algorithms/white_balance.py are imported through oracle.ref_import's cv2 shim.  The
shim's GaussianBlur takes no (0, 0) window and it has no addWeighted, so this tool attaches both for the run: they are
tests/unsharp_restatement.py's -- the window rule in front of oracle.gaussian_blur_fixed, and the float32 addWeighted
[from memory, unpinned].  What the fixtures therefore pin is the reference's own code -- the arguments it gives cv2, the
threshold * 256 for uint16, its thresholded NumPy branch (float32, clip, truncation), the white balance's float64
arithmetic -- on top of restated primitives, as everywhere in this repository.  Data only: input frames, the recorded cv2
calls of every case, the outputs.
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_import  # noqa: E402
import unsharp_restatement as usr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def lowbias32(x):
    """the benchmark's hash generator (csrc/common.hpp lowbias32) on a uint32 array"""
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def synth_edges(h, w, seed, amp=5):
    """uint8 BGR frame: a smooth texture, a nearly white and a nearly black block (edges that saturate when sharpened) and
    integer hash noise in [-amp, amp]"""
    y, x = np.mgrid[:h, :w]
    tex = 120.0 + 60.0 * np.sin(x / 5.0) * np.cos(y / 4.0)
    tex = np.where((x > 0.55 * w) & (y < 0.5 * h), 251.0, tex)
    tex = np.where((x < 0.4 * w) & (y > 0.6 * h), 3.0, tex)
    idx = (np.arange(h * w * 3, dtype=np.uint32) + np.uint32(seed * 7919)).reshape(h, w, 3)
    noise = (lowbias32(idx) % np.uint32(2 * amp + 1)).astype(np.int64) - amp
    img = np.rint(tex).astype(np.int64)[:, :, None] + np.array([4, 0, -3]) + noise
    return np.clip(img, 0, 255).astype(np.uint8)


def widen_u16(img8):
    """The uint16 frame derived from a uint8 frame (integers only, so it is the same everywhere)"""
    a = img8.astype(np.uint32)
    idx = np.arange(a.size, dtype=np.uint32).reshape(a.shape)
    return ((a << 8) | ((a * 37 + idx * 101) & 255)).astype(np.uint16)


def main():
    ref_import.load_pyramid_module()      # the package stubs and the cv2 shim
    cv2 = sys.modules["cv2"]
    calls = []

    def gaussian_blur(src, ksize, sigma):
        out = usr.gaussian_blur(src, ksize, sigma)
        calls.append({"fn": "GaussianBlur", "ksize_arg": list(ksize), "sigma": float(sigma),
                      "ksize": usr.window_size(src.dtype, sigma), "dtype": src.dtype.name})
        return out

    def add_weighted(src1, alpha, src2, beta, gamma):
        calls.append({"fn": "addWeighted", "alpha": float(alpha), "beta": float(beta), "gamma": float(gamma)})
        return usr.add_weighted(src1, alpha, src2, beta, gamma)
    cv2.GaussianBlur, cv2.addWeighted = gaussian_blur, add_weighted
    sh = importlib.import_module("shinestacker.algorithms.sharpen")
    wb = importlib.import_module("shinestacker.algorithms.white_balance")
    assert sh.__file__.startswith(ref_import.REF_SRC) and wb.__file__.startswith(ref_import.REF_SRC)

    frames = {"odd": synth_edges(53, 71, 1), "even": synth_edges(48, 64, 2), "small": synth_edges(20, 24, 3),
              "narrow": synth_edges(40, 7, 4), "tiny": synth_edges(3, 2, 5)}
    arrays = {f"frame_{k}": v for k, v in frames.items()}
    meta = {"unsharp": [], "white_balance": []}
    # (frame, radius, amount, threshold; None = the function's defaults); every case is recorded for both dtypes
    cases = [("odd", r, 0.5, 0) for r in (0.01, 0.25, 1, 2, 3, 4)]
    cases += [("even", 1, 1.5, 0), ("even", 2, 3.0, 0), ("even", 3, 1.5, 10), ("even", 4, 3.0, 64),
              ("odd", 1, 0.5, 10), ("odd", 0.25, 3.0, 0), ("odd", None, None, None), ("odd", 2.5, 1.0, 0),
              ("small", 4, 0.5, 0), ("small", 2, 1.5, 10), ("narrow", 4, 0.5, 0), ("narrow", 4, 3.0, 10),
              ("tiny", 4, 1.5, 0), ("tiny", 1, 0.5, 10)]
    for fr, radius, amount, threshold in cases:
        for wide in (False, True):
            img = widen_u16(frames[fr]) if wide else frames[fr]
            calls.clear()
            out = sh.unsharp_mask(img) if radius is None else sh.unsharp_mask(img, radius, amount, threshold)
            assert out.dtype == img.dtype and out.shape == img.shape and calls[0]["fn"] == "GaussianBlur"
            assert len(calls) == (2 if not threshold else 1)
            name = f"{fr}_{'u16' if wide else 'u8'}_r{radius}_a{amount}_t{threshold}"
            arrays[f"out_{name}"] = out
            meta["unsharp"].append({"name": name, "frame": fr, "u16": wide, "radius": radius, "amount": amount,
                                    "threshold": threshold, "cv2_calls": [dict(c) for c in calls],
                                    "changed_values": int((out != img).sum())})

    # the reference test's target, one with a zero channel, one whose blue scale saturates, and all zero
    for fr, rgb in (("even", (246, 233, 178)), ("even", (0, 200, 100)), ("even", (255, 40, 10)), ("odd", (246, 233, 178)),
                    ("tiny", (0, 0, 0)), ("small", (90.5, 120.25, 200))):
        for wide in (False, True):
            img = widen_u16(frames[fr]) if wide else frames[fr]
            out = wb.white_balance_from_rgb(img, rgb)
            assert out.dtype == img.dtype and out.shape == img.shape
            name = f"{fr}_{'u16' if wide else 'u8'}_" + "_".join(str(v) for v in rgb)
            arrays[f"wb_{name}"] = out
            meta["white_balance"].append({"name": name, "frame": fr, "u16": wide, "target_rgb": list(rgb),
                                          "saturated_values": int((out == np.iinfo(img.dtype).max).sum()),
                                          "changed_values": int((out != img).sum())})

    np.savez_compressed(os.path.join(GOLDEN, "retouch.npz"), **arrays)
    with open(os.path.join(GOLDEN, "retouch.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote retouch.npz", os.path.getsize(os.path.join(GOLDEN, "retouch.npz")), "bytes;", len(meta["unsharp"]), "+",
          len(meta["white_balance"]), "cases")
    for c in meta["unsharp"]:
        print(" ", c["name"], c["cv2_calls"], "changed", c["changed_values"])
    for c in meta["white_balance"]:
        print(" ", c["name"], "saturated", c["saturated_values"], "changed", c["changed_values"])


if __name__ == "__main__":
    main()
