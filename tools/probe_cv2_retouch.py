#!/usr/bin/env python3
"""Compare the two cv2 primitives tests/unsharp_restatement.py states from memory with a real OpenCV, where one is installed.

    python tools/probe_cv2_retouch.py

For every recorded unsharp case of tests/golden/retouch.npz: cv2.GaussianBlur(frame, (0, 0), radius) against the restated
blur, cv2.addWeighted(frame, 1 + amount, blurred, -amount, 0) against the restated float32 rule, and the reference's whole
function (restated) against the recorded output.  Prints the number of differing values per case; changes nothing.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import unsharp_restatement as usr  # noqa: E402


def widen_u16(img8):
    a = img8.astype(np.uint32)
    idx = np.arange(a.size, dtype=np.uint32).reshape(a.shape)
    return ((a << 8) | ((a * 37 + idx * 101) & 255)).astype(np.uint16)


def main():
    try:
        import cv2
    except ImportError:
        print("no cv2 here: nothing compared")
        return 0
    z = np.load(os.path.join(ROOT, "tests", "golden", "retouch.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "retouch.json")) as fh:
        meta = json.load(fh)
    print("OpenCV", cv2.__version__)
    bad = 0
    for c in meta["unsharp"]:
        img = z["frame_" + c["frame"]]
        img = widen_u16(img) if c["u16"] else img
        radius, amount = (1.0, 1.0) if c["radius"] is None else (c["radius"], c["amount"])
        blur_cv, blur_re = cv2.GaussianBlur(img, (0, 0), radius), usr.gaussian_blur(img, (0, 0), radius)
        add_cv = cv2.addWeighted(img, 1.0 + amount, blur_re, -amount, 0)
        add_re = usr.add_weighted(img, 1.0 + amount, blur_re, -amount, 0)
        nb, na = int((blur_cv != blur_re).sum()), int((add_cv != add_re).sum())
        bad += nb + na
        print(f"{c['name']:32s} GaussianBlur differs in {nb:6d} values, addWeighted in {na:6d}")
    print("identical" if bad == 0 else f"{bad} differing values: the restatement does not match this OpenCV build")
    return 0


if __name__ == "__main__":
    sys.exit(main())
