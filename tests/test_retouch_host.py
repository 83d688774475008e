"""CPU: the retouch filters without a GPU -- the NumPy restatement (tests/unsharp_restatement.py) against the fixtures recorded
from the reference's own sharpen.py and white_balance.py (tools/gen_golden_retouch.py), the host tap builder against the
oracle's, the white-balance table against the recorded outputs, self-checks that keep a wrong rounding rule from passing,
and the argument checks of the Python layer and the C ABI.  Every comparison is array_equal."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import unsharp_restatement as usr
from conftest import GOLDEN, load_golden


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "retouch.json")) as fh:
        return load_golden("retouch"), json.load(fh)


def widen_u16(img8):
    """the uint16 frame of a recorded uint8 frame, as tools/gen_golden_retouch.py derives it (integers only)"""
    a = img8.astype(np.uint32)
    idx = np.arange(a.size, dtype=np.uint32).reshape(a.shape)
    return ((a << 8) | ((a * 37 + idx * 101) & 255)).astype(np.uint16)


def case_frame(z, c):
    fr = z["frame_" + c["frame"]]
    return widen_u16(fr) if c["u16"] else fr


def case_args(c):
    return () if c["radius"] is None else (c["radius"], c["amount"], c["threshold"])


def case_values(c):
    """(radius, amount, threshold) with the function's defaults filled in"""
    return (1.0, 1.0, 0.0) if c["radius"] is None else (c["radius"], c["amount"], c["threshold"])


def test_restatement_reproduces_the_recorded_cases(gold):
    """Every recorded case: the cv2 calls the reference made (window (0, 0), sigma = radius, alpha = 1 + amount,
    beta = -amount; no addWeighted in the thresholded branch) and the output."""
    z, meta = gold
    assert len(meta["unsharp"]) >= 36
    radii, amounts, thresholds = set(), set(), set()
    for c in meta["unsharp"]:
        img = case_frame(z, c)
        radius, amount, threshold = case_values(c)
        blur = c["cv2_calls"][0]
        assert blur["fn"] == "GaussianBlur" and blur["ksize_arg"] == [0, 0] and blur["sigma"] == radius
        assert blur["ksize"] == usr.window_size(img.dtype, radius), c["name"]
        if threshold == 0:
            (_, add) = c["cv2_calls"]
            assert (add["fn"], add["alpha"], add["beta"], add["gamma"]) == ("addWeighted", 1.0 + amount, -amount, 0.0)
        else:
            assert len(c["cv2_calls"]) == 1
        out = usr.unsharp_mask(img, *case_args(c))
        assert out.dtype == img.dtype and np.array_equal(out, z["out_" + c["name"]]), c["name"]
        radii.add(radius), amounts.add(amount), thresholds.add(threshold)
    assert radii >= {0.01, 0.25, 1, 2, 3, 4} and amounts >= {0.5, 1.5, 3.0} and thresholds >= {0, 10, 64}
    shapes = {z["frame_" + c["frame"]].shape[:2] for c in meta["unsharp"]}
    assert (40, 7) in shapes and any(h % 2 and w % 2 for h, w in shapes) and any(not h % 2 and not w % 2 for h, w in shapes)
    assert any(h < 32 and w < 32 for h, w in shapes)


def test_window_rule_and_tap_builder_equal_the_oracle(gold, oracle):
    """window_size gives the recorded ksize (0.25 is a cvRound tie for uint8: 2.5 -> 2 -> 3; 0.01 is the identity window);
    gaussian_taps equals oracle.gauss_kernel_fixed for every window the cases use, and sums to exactly 1.0"""
    sh = importlib.import_module("shinestacker_amd.sharpen")
    _, meta = gold
    seen = set()
    for c in meta["unsharp"]:
        dt = np.uint16 if c["u16"] else np.uint8
        radius = case_values(c)[0]
        ksize = sh.window_size(dt, radius)
        assert ksize == c["cv2_calls"][0]["ksize"], c["name"]
        bits = 16 if c["u16"] else 8
        taps = sh.gaussian_taps(dt, ksize, float(radius))
        assert taps.dtype == np.uint32 and np.array_equal(taps, oracle.gauss_kernel_fixed(ksize, float(radius), bits)), c["name"]
        assert int(taps.sum(dtype=np.uint64)) == 1 << bits
        seen.add((bits, ksize))
    assert {(8, 1), (8, 3), (8, 7), (8, 25), (16, 1), (16, 3), (16, 9), (16, 33)} <= seen
    assert sh.window_size(np.uint8, 0.25) == 3 and sh.window_size(np.uint8, 0.01) == 1 and sh.window_size(np.uint16, 4.0) == 33
    assert sh.window_size(np.uint8, 0.75) == 7 and sh.window_size(np.uint8, 0.5) == 5      # 5.5 -> 6 -> 7; 4 -> 5


def test_white_balance_table_equals_every_recorded_output(gold):
    wb = importlib.import_module("shinestacker_amd.white_balance")
    z, meta = gold
    assert len(meta["white_balance"]) >= 10
    targets = set()
    for c in meta["white_balance"]:
        img = case_frame(z, c)
        table = wb.white_balance_table(img.dtype, c["target_rgb"])
        assert table.dtype == img.dtype and table.shape == (3, 256 if img.dtype == np.uint8 else 65536)
        out = np.stack([np.take(table[ch], img[..., ch]) for ch in range(3)], axis=-1)
        assert np.array_equal(out, z["wb_" + c["name"]]), c["name"]
        targets.add(tuple(c["target_rgb"]))
    assert (246, 233, 178) in targets and any(0 in t and any(t) for t in targets)
    assert any(c["saturated_values"] > 1000 for c in meta["white_balance"])
    # a zero channel keeps its values (scale 1.0): R of target (0, 200, 100) is channel 2 of the BGR frame
    t = wb.white_balance_table(np.uint8, (0, 200, 100))
    assert np.array_equal(t[2], np.arange(256, dtype=np.uint8))


def test_fixtures_distinguish_the_rounding_rules(gold):
    """The amount-0.5 addWeighted cases hold exact .5 ties on an even floor (half to even != half up) and on an odd floor
    (half to even != truncation), so the three rules give three different frames; a thresholded case holds values where
    truncation and rounding differ; saturation occurs at 0 and at the maximum; both mask states occur in every
    thresholded case."""
    z, meta = gold
    ties_even = ties_odd = trunc_vs_round = sat_lo = sat_hi = 0
    for c in meta["unsharp"]:
        img = case_frame(z, c)
        radius, amount, threshold = case_values(c)
        maxv = np.iinfo(img.dtype).max
        blurred = usr.gaussian_blur(img, (0, 0), radius)
        fi, fb = img.astype(np.float32), blurred.astype(np.float32)
        if threshold == 0:
            s = fi * np.float32(1.0 + amount) + fb * np.float32(-amount)
            assert s.dtype == np.float32
            inside = (s > 0) & (s < maxv)
            tie = inside & (s - np.floor(s) == 0.5)
            if amount == 0.5 and radius >= 1:
                even, odd = int((tie & (np.floor(s) % 2 == 0)).sum()), int((tie & (np.floor(s) % 2 == 1)).sum())
                assert even > 0 and odd > 0, c["name"]
                ties_even, ties_odd = ties_even + even, ties_odd + odd
                half_even = np.clip(np.rint(s), 0, maxv)
                half_up = np.clip(np.floor(s + np.float32(0.5)), 0, maxv)
                trunc = np.clip(np.trunc(s), 0, maxv)
                assert not np.array_equal(half_even, half_up) and not np.array_equal(half_even, trunc)
                assert not np.array_equal(half_up, trunc)
            sat_lo, sat_hi = sat_lo + int((s < 0).sum()), sat_hi + int((s > maxv).sum())
        else:
            thr = np.float32(threshold * (256 if c["u16"] else 1))
            diff = fi - fb
            mask = np.abs(diff) > thr
            assert mask.any() and not mask.all(), c["name"]
            val = fi + np.float32(amount) * diff
            inside = mask & (val > 0) & (val < maxv)
            trunc_vs_round += int((inside & (np.trunc(val) != np.rint(val))).sum())
            sat_lo, sat_hi = sat_lo + int((mask & (val < 0)).sum()), sat_hi + int((mask & (val > maxv)).sum())
    assert ties_even > 100 and ties_odd > 100 and trunc_vs_round > 100 and sat_lo > 100 and sat_hi > 100


def test_identity_window_and_constant_frame():
    """ksize 1 is the identity blur, so image - blurred == 0 and both branches return the input; a constant frame too"""
    img = (np.arange(5 * 7 * 3) * 37 % 256).astype(np.uint8).reshape(5, 7, 3)
    for frame in (img, widen_u16(img)):
        assert np.array_equal(usr.unsharp_mask(frame, 0.01, 3.0, 0), frame)
        assert np.array_equal(usr.unsharp_mask(frame, 0.01, 3.0, 10), frame)
    flat = np.full((9, 11, 3), 200, np.uint8)
    assert np.array_equal(usr.unsharp_mask(flat, 4, 3.0, 0), flat)


def test_python_argument_checks():
    from shinestacker_amd import BitDepthError, InvalidOptionError, unsharp_mask, white_balance_from_rgb
    sh = importlib.import_module("shinestacker_amd.sharpen")
    wb = importlib.import_module("shinestacker_amd.white_balance")
    img = np.zeros((8, 8, 3), np.uint8)
    for fn, args in ((unsharp_mask, ()), (white_balance_from_rgb, ((246, 233, 178),))):
        with pytest.raises(BitDepthError):
            fn(img.astype(np.float32), *args)
        for bad in (img[..., 0], img[..., :2], np.zeros((0, 8, 3), np.uint8)):
            with pytest.raises(InvalidOptionError):
                fn(bad, *args)
    for bad_radius in (0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(InvalidOptionError):
            unsharp_mask(img, bad_radius)
    with pytest.raises(InvalidOptionError):      # uint8: cvRound(4.5 * 6 + 1) | 1 = 29 fits, 5.5 -> 35 does not
        unsharp_mask(img, 5.5)
    with pytest.raises(InvalidOptionError):      # uint16: cvRound(4.1 * 8 + 1) | 1 = 35
        unsharp_mask(img.astype(np.uint16), 4.1)
    assert sh.window_size(np.uint8, 4.5) == 29 and sh.MAX_KSIZE == 33
    for kw in ({"amount": float("nan")}, {"threshold": float("inf")}, {"amount": "1"}):
        with pytest.raises(InvalidOptionError):
            unsharp_mask(img, 1.0, **kw)
    for bad_rgb in ((1, 2), (1, 2, 3, 4), 5, (1, "2", 3), (1, float("nan"), 3)):
        with pytest.raises(InvalidOptionError):
            white_balance_from_rgb(img, bad_rgb)
        with pytest.raises(InvalidOptionError):
            wb.white_balance_table(np.uint8, bad_rgb)
    with pytest.raises(BitDepthError):
        sh.unsharp_mask_device(1, 2, 8, 8, np.float32)
    with pytest.raises(BitDepthError):
        wb.white_balance_device(1, 2, 64, np.float32, (1, 2, 3))
    import shinestacker_amd
    assert "unsharp_mask" in shinestacker_amd.__all__ and "white_balance_from_rgb" in shinestacker_amd.__all__


def test_pipeline_refuses_bad_retouch_options_before_touching_the_device():
    from shinestacker_amd import InvalidOptionError
    from shinestacker_amd.pipeline import align_and_stack, align_and_stack_device, bunches_then_stack
    frames = [np.zeros((64, 64, 3), np.uint8)]
    for kw in ({"unsharp": (0, 1.0, 0)}, {"unsharp": (1.0, 1.0)}, {"unsharp": 1.0}, {"unsharp": (5.5, 1.0, 0)},
               {"white_balance": (1, 2)}, {"white_balance": (1, 2, float("nan"))}):
        with pytest.raises(InvalidOptionError):
            align_and_stack(frames, **kw)
        with pytest.raises(InvalidOptionError):
            align_and_stack_device(0, 1, 64, 64, np.uint8, **kw)
        with pytest.raises(InvalidOptionError):
            bunches_then_stack(lambda i: None, 4, 64, 64, np.uint8, **kw)
    with pytest.raises(InvalidOptionError):      # 33 taps hold radius 4 on uint16, not 4.1
        align_and_stack_device(0, 1, 64, 64, np.uint16, unsharp=(4.1, 1.0, 0))


def test_argument_validation_without_gpu(hiplib):
    """mi_unsharp_mask / mi_unsharp_mask_device refuse bad arguments before any device call"""
    sh = importlib.import_module("shinestacker_amd.sharpen")
    lib = hiplib.load()
    taps = sh.gaussian_taps(np.uint8, 7, 1.0)
    img = np.zeros((8, 8, 3), np.uint8)
    out = np.zeros_like(img)
    tp, ip, op = taps.ctypes.data, img.ctypes.data, out.ctypes.data
    INV = hiplib.MI_ERR_INVALID
    assert lib.mi_unsharp_mask(0, None, op, 8, 8, hiplib.MI_U8, tp, 7, 1.0, 0.0) == INV and b"null" in lib.mi_last_error()
    assert lib.mi_unsharp_mask(0, ip, None, 8, 8, hiplib.MI_U8, tp, 7, 1.0, 0.0) == INV
    assert lib.mi_unsharp_mask(0, ip, op, 8, 8, hiplib.MI_U8, None, 7, 1.0, 0.0) == INV
    assert lib.mi_unsharp_mask(0, ip, op, 8, 8, hiplib.MI_F32, tp, 7, 1.0, 0.0) == INV
    assert lib.mi_unsharp_mask(0, ip, op, 0, 8, hiplib.MI_U8, tp, 7, 1.0, 0.0) == INV
    assert lib.mi_unsharp_mask(0, ip, op, 8, 8, hiplib.MI_U8, tp, 6, 1.0, 0.0) == INV and b"ksize" in lib.mi_last_error()
    big = np.zeros(35, np.uint32)
    big[17] = 256
    assert lib.mi_unsharp_mask(0, ip, op, 8, 8, hiplib.MI_U8, big.ctypes.data, 35, 1.0, 0.0) == INV and b"ksize" in lib.mi_last_error()
    assert lib.mi_unsharp_mask(0, ip, op, 8, 8, hiplib.MI_U8, tp, 0, 1.0, 0.0) == INV
    assert lib.mi_unsharp_mask(0, ip, op, 8, 8, hiplib.MI_U16, tp, 7, 1.0, 0.0) == INV and b"sum" in lib.mi_last_error()   # 8-bit taps
    assert lib.mi_unsharp_mask(0, ip, op, 8, 8, hiplib.MI_U8, tp, 7, float("nan"), 0.0) == INV
    # the device entry point: src == dst is refused (every output reads a neighbourhood of inputs)
    assert lib.mi_unsharp_mask_device(0, None, ip, ip, 8, 8, hiplib.MI_U8, tp, 7, 1.0, 0.0) == INV and b"differ" in lib.mi_last_error()
    assert lib.mi_unsharp_mask_device(0, None, ip, None, 8, 8, hiplib.MI_U8, tp, 7, 1.0, 0.0) == INV
    assert lib.mi_unsharp_mask_device(0, None, ip, op, 8, 8, hiplib.MI_U8, tp, 8, 1.0, 0.0) == INV
    for name in ("mi_unsharp_mask", "mi_unsharp_mask_device"):
        assert name in hiplib.SIGNATURES and hasattr(C.CDLL(hiplib.LIB_PATH), name)


@pytest.mark.skipif(os.environ.get("MI_EXPECT_GPU") == "1", reason="GPU box")
def test_no_gpu_means_device_error(hiplib):
    if hiplib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    from shinestacker_amd import DeviceError, unsharp_mask, white_balance_from_rgb
    from shinestacker_amd.sharpen import unsharp_mask_device
    from shinestacker_amd.white_balance import white_balance_device
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(DeviceError):
        unsharp_mask(img, 1.0, 0.5, 10)
    with pytest.raises(DeviceError):
        white_balance_from_rgb(img, (246, 233, 178))
    with pytest.raises(DeviceError):
        unsharp_mask_device(1, 2, 8, 8, np.uint8)
    with pytest.raises(DeviceError):
        white_balance_device(1, 1, 64, np.uint8, (246, 233, 178))
