#!/usr/bin/env python3
"""Record tests/golden/prestack.npz + prestack.json from the reference's OWN Vignetting, MaskNoise and NoiseDetection code.

    python tools/gen_golden_prestack.py          (needs the reference tree; see oracle/ref_import.py)

The reference's algorithms/vignetting.py and algorithms/noise_detection.py are imported through oracle.ref_import (the
cv2 shim supplies the integer BGR2GRAY and the INTER_AREA resize; parity for those two OpenCV primitives is unpinned, as
everywhere in this repository).  Float64 `np.exp` inside vignetting.py goes through ref_import._NumpyWithExactExp (long
double, rounded once), so the recorded corrected frames do not depend on the NumPy build's SIMD exp.

Recorded: input frames, ring radii / means, fitted parameters, v0, percentile radii, corrected frames (vignetting);
hot-pixel coordinates and the corrected values at them (mask noise); constructor signatures.  Data only.
"""
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

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


def synth_vignetted(h, w, seed, k_rel=6.0, r0_rel=0.75):
    """uint8 BGR frame: a known double-exponential sigmoid of the radius times a smooth texture, plus integer hash noise"""
    y, x = np.ogrid[:h, :w]
    r = np.sqrt((x - w / 2)**2 + (y - h / 2)**2)
    r_max = np.sqrt((w / 2)**2 + (h / 2)**2)
    fall = 2.0 / (1.0 + np.exp(np.minimum(10, np.exp(np.clip(k_rel / r_max * (r - r0_rel * r_max), -10, 10)))))
    fall = fall / fall.max()
    tex = 0.85 + 0.15 * np.sin(x / 17.0) * np.cos(y / 23.0)
    idx = (np.arange(h * w * 3, dtype=np.uint32) + np.uint32(seed * 7919)).reshape(h, w, 3)
    noise = (lowbias32(idx) % np.uint32(9)).astype(np.int64) - 4
    base = np.array([150.0, 200.0, 175.0])[None, None, :]
    img = np.rint(base * (fall * tex)[:, :, None]).astype(np.int64) + noise
    return np.clip(img, 0, 255).astype(np.uint8)


def widen_u16(img8):
    """The uint16 frame the tests derive from a recorded uint8 frame (integers only, so it is the same everywhere)"""
    a = img8.astype(np.uint32)
    idx = np.arange(a.size, dtype=np.uint32).reshape(a.shape)
    return ((a << 8) | ((a * 37 + idx * 101) & 255)).astype(np.uint16)


class Proc(ref_import.FakeProcess):
    counts = 1
    working_path = "."
    plot_path = "plots"

    def sub_message(self, *_a, **_k):
        pass


def signature_of(cls):
    out = []
    for p in list(inspect.signature(cls.__init__).parameters.values())[1:]:
        out.append({"name": p.name, "kind": p.kind.name, "has_default": p.default is not inspect.Parameter.empty,
                    "default": None if p.default is inspect.Parameter.empty else repr(p.default)})
    return out


def main():
    ref_import.load_balance_module()   # pyramid + the stubs for exif / denoise / matplotlib + config
    import importlib
    plt = sys.modules["matplotlib.pyplot"]
    for name in ("figure", "plot", "savefig", "close", "xlabel", "ylabel", "legend", "xlim", "ylim", "fill_between"):
        if not hasattr(plt, name):
            setattr(plt, name, lambda *a, **k: None)
    vig = importlib.import_module("shinestacker.algorithms.vignetting")
    vig.np = ref_import._NumpyWithExactExp()
    arrays, meta = {}, {"vignetting": [], "mask_noise": [], "signatures": {}}

    # ---- vignetting
    frame_a = synth_vignetted(203, 301, 1)              # odd sizes: w / 2, h / 2 fractional
    frame_b = synth_vignetted(240, 320, 2, 5.0, 0.7)    # even sizes
    frame_b[228:, :] = 0                                # a black bar under black_threshold ...
    frame_b[:6, :, 1] = 0                               # ... and a strip where only one channel is black
    frame_c = synth_vignetted(120, 160, 3, 7.0, 0.8)    # small: the corrected 16-bit frame stays small too
    frame_c[110:, :40] = 0
    arrays["frame_a"], arrays["frame_b"], arrays["frame_c"] = frame_a, frame_b, frame_c
    frames = {"a": frame_a, "b": frame_b, "c": frame_c}
    cases = [
        # (name, frame, 16-bit, subsample, fast, r_steps, max_correction, black_threshold, keep the corrected frame)
        ("a_u8_s8", "a", False, 8, False, 100, 1, 1.0, False),
        ("a_u8_s8_fast", "a", False, 8, True, 100, 1, 1.0, False),
        ("a_u8_s2", "a", False, 2, False, 100, 1, 1.0, False),
        ("a_u8_s2_fast", "a", False, 2, True, 100, 1, 1.0, False),
        ("a_u8_s1", "a", False, 1, False, 100, 1, 1.0, True),
        ("a_u8_s3_r37", "a", False, 3, False, 37, 0.6, 1.0, False),
        ("a_u16_s8", "a", True, 8, False, 100, 1, 1.0, False),
        ("a_u16_s1", "a", True, 1, False, 64, 1, 1.0, False),
        ("b_u8_s8", "b", False, 8, False, 100, 1, 1.0, False),
        ("b_u8_s2_mc06", "b", False, 2, False, 100, 0.6, 1.0, True),
        ("b_u16_s2", "b", True, 2, False, 100, 1, 1.0, False),
        ("b_u16_s8_fast", "b", True, 8, True, 50, 1, 1.0, False),
        ("c_u8_s2_bt20", "c", False, 2, False, 60, 1, 20.0, True),
        ("c_u16_s2", "c", True, 2, False, 60, 1, 1.0, False),
        ("c_u16_s1_mc06", "c", True, 1, True, 60, 0.6, 4.0, True),
    ]
    for name, fr, wide, sub, fast, r_steps, mc, bt, keep in cases:
        img = widen_u16(frames[fr]) if wide else frames[fr]
        image_sub = vig.img_subsampled(img, sub, fast)
        radii, means = vig.radial_mean_intensity(image_sub, r_steps)
        hs, ws = image_sub.shape
        table = np.linspace(0, np.sqrt((ws / 2)**2 + (hs / 2)**2), r_steps + 1)
        params = vig.compute_fit_parameters(img, r_steps, radii, means, sub, fast)
        action = vig.Vignetting(r_steps=r_steps, max_correction=mc, black_threshold=bt, subsample=sub, fast_subsampling=fast)
        action.begin(Proc())
        out = action.run_frame(0, 0, img)
        assert out.dtype == img.dtype and out.shape == img.shape
        arrays[f"v_{name}_table"] = table
        arrays[f"v_{name}_radii"] = radii
        arrays[f"v_{name}_means"] = means
        arrays[f"v_{name}_params"] = np.asarray(params, np.float64)
        arrays[f"v_{name}_v0"] = np.float64(action.v0)
        arrays[f"v_{name}_percentile_radii"] = np.array([c[0] for c in action.corrections], np.float64)
        rows = None
        if keep:
            # the 240-row frame keeps its one-channel strip, a band through the centre and the black bar only
            rows = [0, 10, 100, 140, 222, 240] if fr == "b" else [0, img.shape[0]]
            arrays[f"v_{name}_out"] = np.concatenate([out[a:b] for a, b in zip(rows[::2], rows[1::2])])
        meta["vignetting"].append({"name": name, "frame": fr, "u16": wide, "subsample": sub, "fast_subsampling": fast,
                                   "r_steps": r_steps, "max_correction": mc, "black_threshold": bt, "has_out": keep, "out_rows": rows,
                                   "sub_shape": [int(hs), int(ws)], "percentiles": [float(p) for p in action.percentiles],
                                   "changed_values": int((out != img).sum())})

    # ---- mask noise
    nd = importlib.import_module("shinestacker.algorithms.noise_detection")
    base = synth_vignetted(96, 128, 4)
    h, w = base.shape[:2]
    hot = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (10, 10), (10, 11), (11, 10), (40, 64), (41, 65), (0, 50), (57, 0),
           (70, 100), (70, 102), (95, 77)]
    mask = np.zeros((h, w), np.uint8)
    for i, (y, x) in enumerate(hot):
        mask[y, x] = 255 if i % 2 == 0 else 1 + i          # any non-zero value is hot
        base[y, x] = (255, 250 - i, 255)
    base[40, 63] = 0                                        # a zero-valued neighbour (all channels)
    base[69, 101, 1] = 0                                    # ... and one in a single channel
    base[20:23, 30:33] = 0                                  # a hot pixel whose whole 3 x 3 window is zero: unchanged for kernel 3
    mask[21, 31] = 9
    arrays["mn_frame"], arrays["mn_mask"] = base, mask
    coords = np.argwhere(mask > 0)
    for wide in (False, True):
        img = widen_u16(base) if wide else base
        if wide:
            img[20:23, 30:33] = 0
            img[40, 63] = 0
            img[69, 101, 1] = 0
        for ks in (3, 5):
            for method in ("MEAN", "MEDIAN"):
                action = nd.MaskNoise(kernel_size=ks, method=method)
                action.process = Proc()
                action.noise_mask_img = mask
                out = action.run_frame(0, 0, img)
                assert out.dtype == img.dtype
                changed = np.any(out != img, axis=2)
                assert not np.any(changed & (mask == 0)), "the reference touched a pixel outside the mask"
                name = f"{'u16' if wide else 'u8'}_k{ks}_{method.lower()}"
                arrays[f"mn_{name}_values"] = out[coords[:, 0], coords[:, 1]]
                meta["mask_noise"].append({"name": name, "u16": wide, "kernel_size": ks, "method": method})
    arrays["mn_coords"] = coords.astype(np.int32)
    meta["mask_noise_zeroed"] = [[20, 23, 30, 33, -1], [40, 41, 63, 64, -1], [69, 70, 101, 102, 1]]   # y0, y1, x0, x1, channel

    # ---- noise detection: the reference's NoiseDetection.run_core on files that exist only by name (read_img looks the
    # frames up), over a cv2 stand-in that adds, for this module only, the exact integer calls the shim lacks
    import tempfile
    import types
    small = {3: [1, 2, 1], 5: [1, 4, 6, 4, 1], 7: [2, 7, 14, 18, 14, 7, 2]}

    def gaussian_blur_small(img, ksize, sigma):
        """cv2.GaussianBlur(uint8, (k, k), 0), k = 3 / 5 / 7 [from memory]: the fixed small kernel in 8.8 fixed point"""
        assert ksize[0] == ksize[1] and sigma == 0 and img.dtype == np.uint8
        wt = np.array(small[ksize[0]], np.int64)
        f = 256 // wt.sum()
        r = ksize[0] // 2
        pad = np.pad(img.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="reflect")
        acc = np.zeros(img.shape, np.int64)
        for j in range(ksize[0]):
            for i in range(ksize[0]):
                acc += wt[j] * wt[i] * pad[j:j + img.shape[0], i:i + img.shape[1]]
        return ((acc * f * f + (1 << 15)) >> 16).astype(np.uint8)
    written = {}
    real_cv2 = sys.modules["cv2"]
    cv2x = types.SimpleNamespace(**{k: getattr(real_cv2, k) for k in dir(real_cv2) if not k.startswith("__")})
    cv2x.THRESH_BINARY = 0
    cv2x.GaussianBlur = gaussian_blur_small
    cv2x.absdiff = lambda a, b: np.abs(a.astype(np.int16) - b.astype(np.int16)).astype(np.uint8)
    cv2x.threshold = lambda ch, th, maxval, kind: (float(th), np.where(ch > th, maxval, 0).astype(np.uint8))
    cv2x.bitwise_or = lambda a, b: a | b
    cv2x.imwrite = lambda path, img: written.__setitem__(path, img.copy()) or True
    nd.cv2 = cv2x
    nh, nw, n_noise = 75, 102, 7
    noise_frames = []
    planted = [(0, 0), (0, nw - 1), (nh - 1, 0), (nh - 1, nw - 1), (20, 30), (20, 31), (40, 50), (41, 50), (60, 7), (33, 90), (5, 70)]
    for f in range(n_noise):
        fr = synth_vignetted(nh, nw, 20 + f)
        for k, (y, x) in enumerate(planted):
            fr[y, x, k % 3] = min(255, int(fr[y, x, k % 3]) + 40 + 9 * k)     # hot in one channel ...
            if k % 4 == 0:
                fr[y, x] = 250                                                # ... or in all three
        noise_frames.append(fr)
    arrays["nd_frames"] = np.stack(noise_frames)
    nd.read_img = lambda path: noise_frames[int(os.path.basename(path)[1:4])].copy()
    meta["noise_detection"] = []
    for name, opts in (("all", {}), ("max1", {"max_frames": 1}), ("max3", {"max_frames": 3}),
                       ("blur3_th", {"blur_size": 3, "channel_thresholds": [9, 13, 20]}), ("blur7", {"blur_size": 7})):
        with tempfile.TemporaryDirectory() as work:
            os.makedirs(os.path.join(work, "frames"))
            for f in range(n_noise):
                open(os.path.join(work, "frames", f"f{f:03d}.png"), "wb").close()
            trace = []
            action = nd.NoiseDetection("noise-map", input_path="frames", **opts)
            action.id = 0
            action.print_message = action.print_message_r = lambda *a, **k: None      # console logging only
            action.callbacks = {k: (lambda *a, k=k: trace.append([k, *a[2:]]) or True) for k in ("step_counts", "after_step", "check_running")}
            job = types.SimpleNamespace(working_path=work, paths=["frames"], name="job")
            action.init(job)
            real_list = action.folder_filelist
            action.folder_filelist = lambda: sorted(real_list())       # os.walk order is arbitrary; the mirror sorts
            written.clear()
            action.run_core()
            (path, hot_rgb), = written.items()
            assert path == f"{work}/noise-map/hot_pixels.png" and os.path.isdir(os.path.join(work, "noise-map"))
        counter = n_noise if opts.get("max_frames", -1) < 1 else min(n_noise, opts["max_frames"] + 1)
        mean = (np.stack(noise_frames[:counter]).astype(np.float64).sum(axis=0) / counter).astype(np.uint8)
        blurred = gaussian_blur_small(mean, (opts.get("blur_size", 5),) * 2, 0)
        diff = cv2x.absdiff(mean, blurred)
        th = opts.get("channel_thresholds", [13, 13, 13])
        per_ch = [int((diff[..., c] > th[c]).sum()) for c in range(3)]
        assert np.array_equal(hot_rgb > 0, np.any(diff > np.array(th), axis=2))      # the recorded mean is the one the map came from
        if "max_frames" in opts or name == "all":      # the other cases average the same frames as "all"
            arrays[f"nd_{name}_mean"] = mean
        arrays[f"nd_{name}_map"] = hot_rgb
        meta["noise_detection"].append({"name": name, "options": opts, "frames_averaged": counter, "trace": trace,
                                        "counts": [int((hot_rgb > 0).sum())] + per_ch, "file_name": "noise-map/hot_pixels.png"})

    meta["signatures"] = {"Vignetting": signature_of(vig.Vignetting), "MaskNoise": signature_of(nd.MaskNoise),
                          "NoiseDetection": signature_of(nd.NoiseDetection)}
    meta["constants"] = {k: getattr(vig.constants, k) for k in (
        "DEFAULT_R_STEPS", "DEFAULT_BLACK_THRESHOLD", "DEFAULT_MAX_CORRECTION", "DEFAULT_VIGN_SUBSAMPLE",
        "DEFAULT_VIGN_FAST_SUBSAMPLING", "DEFAULT_NOISE_MAP_FILENAME", "DEFAULT_MN_KERNEL_SIZE", "INTERPOLATE_MEAN",
        "INTERPOLATE_MEDIAN")}
    meta["constants"]["VALID_INTERPOLATE"] = sorted(vig.constants.VALID_INTERPOLATE)
    meta["constants"]["MAX_NOISY_PIXELS"] = nd.MAX_NOISY_PIXELS
    meta["constants"]["CLIP_EXP"] = vig.CLIP_EXP
    np.savez_compressed(os.path.join(GOLDEN, "prestack.npz"), **arrays)
    with open(os.path.join(GOLDEN, "prestack.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote prestack.npz", os.path.getsize(os.path.join(GOLDEN, "prestack.npz")), "bytes;",
          len(meta["vignetting"]), "vignetting cases,", len(meta["mask_noise"]), "mask-noise cases")
    for c in meta["vignetting"]:
        print(" ", c["name"], "params", arrays[f"v_{c['name']}_params"], "nan rings", int(np.isnan(arrays[f"v_{c['name']}_means"]).sum()),
              "changed", c["changed_values"])


if __name__ == "__main__":
    main()
