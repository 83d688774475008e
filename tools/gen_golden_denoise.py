#!/usr/bin/env python3
"""Record tests/golden/denoise.npz + denoise.json from the reference's OWN denoise wrapper and stack action.

    python tools/gen_golden_denoise.py          (needs the reference tree; see oracle/ref_import.py)

The reference's algorithms/denoise.py and algorithms/stack.py are imported through oracle.ref_import's cv2 shim.  The shim
lists fastNlMeansDenoising as unavailable, so this tool attaches it (with NORM_L1 / NORM_L2) for the run: the function is
tests/nlm_restatement.py, the NumPy statement of OpenCV's rule [from memory, unpinned].  What the fixtures therefore pin is
the reference's own code -- which norm it picks, the `h` it passes for uint16, the argument order, and that FocusStackBase
passes the amount as filter strength AND template window size -- on top of a restated primitive, as everywhere in this
repository.  Data only: input frames, the recorded cv2 call of every case, the outputs.
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
import nlm_restatement as nlm  # noqa: E402

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


def synth_noisy(h, w, seed, amp=6):
    """uint8 BGR frame: a smooth texture with an edge, plus integer hash noise in [-amp, amp]"""
    y, x = np.mgrid[:h, :w]
    tex = 120.0 + 60.0 * np.sin(x / 9.0) * np.cos(y / 7.0) + 40.0 * (x > 0.6 * w)
    idx = (np.arange(h * w * 3, dtype=np.uint32) + np.uint32(seed * 7919)).reshape(h, w, 3)
    noise = (lowbias32(idx) % np.uint32(2 * amp + 1)).astype(np.int64) - amp
    img = np.rint(tex).astype(np.int64)[:, :, None] + np.array([12, 0, -12]) + noise
    return np.clip(img, 0, 255).astype(np.uint8)


def widen_u16(img8):
    """The uint16 frame derived from a uint8 frame (integers only, so it is the same everywhere)"""
    a = img8.astype(np.uint32)
    idx = np.arange(a.size, dtype=np.uint32).reshape(a.shape)
    return ((a << 8) | ((a * 37 + idx * 101) & 255)).astype(np.uint16)


def main():
    ref_import.load_balance_module()      # pyramid + config + the stubs for exif / denoise / matplotlib
    cv2 = sys.modules["cv2"]
    calls = []

    def fast_nl_means_denoising(src, h, dst, template_window_size, search_window_size, norm_type):
        assert dst is None and len(h) == 1
        calls.append({"h": float(h[0]), "template": template_window_size, "search": search_window_size, "norm": int(norm_type),
                      "dtype": src.dtype.name})
        return nlm.fast_nl_means(src, h[0], template_window_size, search_window_size, norm_type)
    cv2.fastNlMeansDenoising, cv2.NORM_L1, cv2.NORM_L2 = fast_nl_means_denoising, nlm.NORM_L1, nlm.NORM_L2
    del sys.modules["shinestacker.algorithms.denoise"]       # ref_import's stub; the real module is what is recorded
    dn = importlib.import_module("shinestacker.algorithms.denoise")
    assert dn.__file__.startswith(ref_import.REF_SRC)

    frames = {"odd": synth_noisy(67, 91, 1), "even": synth_noisy(64, 96, 2), "small": synth_noisy(20, 24, 3),
              "narrow": synth_noisy(40, 7, 4), "tiny": synth_noisy(3, 2, 5)}
    arrays = {f"frame_{k}": v for k, v in frames.items()}
    meta = {"cases": [], "stack_calls": [], "norm_codes": {"NORM_L1": nlm.NORM_L1, "NORM_L2": nlm.NORM_L2}}
    cases = [
        # (frame, 16-bit, h_luminance, template, search; None = the wrapper's defaults)
        ("odd", False, 3, None, None), ("odd", True, 3, None, None),
        ("even", False, 10, 7, 21), ("even", True, 10, 7, 21),
        ("odd", False, 1, 1, 21), ("odd", True, 1, 1, 21),
        ("even", False, 3, 3, 21), ("even", True, 3, 3, 21),
        ("small", False, 3, 5, 5), ("small", True, 3, 5, 5),
        ("small", False, 10, 11, 21), ("small", True, 10, 11, 21),
        ("narrow", False, 3, 7, 21), ("narrow", True, 3, 7, 21),
        ("tiny", False, 10, 7, 21), ("tiny", True, 10, 7, 21),
        ("even", False, 3, 4, 6), ("even", True, 7.5, 10, 20),       # even windows are forced odd; a non-integral h
    ]
    for fr, wide, h, tpl, srch in cases:
        img = widen_u16(frames[fr]) if wide else frames[fr]
        calls.clear()
        out = dn.denoise(img, h) if tpl is None else dn.denoise(img, h, tpl, srch)
        assert out.dtype == img.dtype and out.shape == img.shape and len(calls) == 1
        name = f"{fr}_{'u16' if wide else 'u8'}_h{h}_t{tpl}_s{srch}"
        arrays[f"out_{name}"] = out
        meta["cases"].append({"name": name, "frame": fr, "u16": wide, "h_luminance": h, "template": tpl, "search": srch,
                              "cv2_call": dict(calls[0]), "changed_values": int((out != img).sum())})

    # FocusStackBase.focus_stack (stack.py:26-52) with a stubbed stacker and writer: what it passes to denoise()
    st = importlib.import_module("shinestacker.algorithms.stack")
    assert st.denoise is dn.denoise
    stacked = frames["small"]
    for amount in (0, 1, 3, 4):
        written, trace = {}, []
        st.write_img = lambda path, img: written.__setitem__(os.path.basename(path), img.copy())

        class Algo:
            process = None

            def focus_stack(self, files):
                return stacked.copy()

            def name(self):
                return "stub"
        action = object.__new__(st.FocusStackBase)
        action.stack_algo, action.exif_path, action.prefix, action.denoise_amount = Algo(), '', 'stack_', amount
        action.plot_stack, action.frame_count, action.input_full_path, action.output_dir = False, -1, "in", "out"
        action.sub_message_r = lambda msg, *a, **k: trace.append(msg)
        calls.clear()
        action.focus_stack(["a.tif", "b.tif"])
        (fname, out), = written.items()
        assert fname == "stack_a.tif"
        if amount:
            arrays[f"stack_amount{amount}"] = out
        else:
            assert np.array_equal(out, stacked) and not calls
        meta["stack_calls"].append({"amount": amount, "cv2_calls": [dict(c) for c in calls],
                                    "messages": [m for m in trace if "denoise" in m], "n_messages": len(trace)})

    np.savez_compressed(os.path.join(GOLDEN, "denoise.npz"), **arrays)
    with open(os.path.join(GOLDEN, "denoise.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote denoise.npz", os.path.getsize(os.path.join(GOLDEN, "denoise.npz")), "bytes;", len(meta["cases"]), "cases")
    for c in meta["cases"]:
        print(" ", c["name"], c["cv2_call"], "changed", c["changed_values"])
    for c in meta["stack_calls"]:
        print("  stack amount", c["amount"], c["cv2_calls"], c["messages"])


if __name__ == "__main__":
    main()
