"""CPU: the post-stack denoise without a GPU -- the NumPy restatement (tests/nlm_restatement.py) against the fixtures recorded
from the reference's own wrapper and stack action (tools/gen_golden_denoise.py), properties of any correct non-local means,
the package's table builder against the restatement's, the stack action's option, and the C ABI's argument checks."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import nlm_restatement as nlm
from conftest import GOLDEN, load_golden


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "denoise.json")) as fh:
        return load_golden("denoise"), json.load(fh)


def widen_u16(img8):
    """the uint16 frame of a recorded uint8 frame, as tools/gen_golden_denoise.py derives it (integers only)"""
    a = img8.astype(np.uint32)
    idx = np.arange(a.size, dtype=np.uint32).reshape(a.shape)
    return ((a << 8) | ((a * 37 + idx * 101) & 255)).astype(np.uint16)


def case_frame(z, c):
    fr = z["frame_" + c["frame"]]
    return widen_u16(fr) if c["u16"] else fr


def case_args(c):
    return (c["h_luminance"],) if c["template"] is None else (c["h_luminance"], c["template"], c["search"])


def hash_noise(shape, seed, amp):
    idx = np.arange(int(np.prod(shape)), dtype=np.uint32) + np.uint32(seed * 7919)
    idx ^= idx >> np.uint32(16)
    idx *= np.uint32(0x7feb352d)
    idx ^= idx >> np.uint32(15)
    idx *= np.uint32(0x846ca68b)
    idx ^= idx >> np.uint32(16)
    return (idx % np.uint32(2 * amp + 1)).astype(np.int64).reshape(shape) - amp


def test_restatement_reproduces_the_recorded_cases(gold):
    """Every recorded case: the wrapper's decisions (norm, h * 256 for uint16, argument order, defaults 7 / 21) and the output."""
    z, meta = gold
    assert len(meta["cases"]) >= 16
    for c in meta["cases"]:
        img = case_frame(z, c)
        call = c["cv2_call"]
        assert call["norm"] == (nlm.NORM_L1 if c["u16"] else nlm.NORM_L2), c["name"]
        assert call["h"] == c["h_luminance"] * (256 if c["u16"] else 1), c["name"]
        assert (call["template"], call["search"]) == ((7, 21) if c["template"] is None else (c["template"], c["search"]))
        out = nlm.denoise(img, *case_args(c))
        assert out.dtype == img.dtype and np.array_equal(out, z["out_" + c["name"]]), c["name"]


def test_stack_action_passes_the_amount_as_strength_and_template_size(gold):
    """stack.py:33-35 as recorded: denoise(stacked, amount, amount) -- h = amount, template = amount, search 21; nothing at 0"""
    z, meta = gold
    by_amount = {c["amount"]: c for c in meta["stack_calls"]}
    assert by_amount[0]["cv2_calls"] == [] and by_amount[0]["messages"] == []
    for amount in (1, 3, 4):
        c = by_amount[amount]
        assert c["messages"] == [": denoise image"]
        (call,) = c["cv2_calls"]
        assert (call["h"], call["template"], call["search"], call["norm"]) == (float(amount), amount, 21, nlm.NORM_L2)
        assert np.array_equal(nlm.denoise(z["frame_small"], amount, amount), z[f"stack_amount{amount}"])


def test_constant_frame_comes_back_identical():
    for dt, v in ((np.uint8, (7, 130, 255)), (np.uint16, (0, 40000, 65535))):
        img = np.empty((23, 31, 3), dt)
        img[:] = v
        for h, tpl, srch in ((3, 7, 21), (10, 3, 5)):
            assert np.array_equal(nlm.denoise(img, h, tpl, srch), img)


def test_vanishing_strength_returns_the_input():
    """h so small that the table is [fpm, 0, 0, ...], on a frame whose patches all differ by more than one table step:
    only the pixel itself has weight."""
    base = (hash_noise((30, 41, 3), 3, 100) + 128).astype(np.uint8)
    # entry 1 is dist = 64 / 49: exp(-dist / (3 h^2)) [L2] and exp(-dist^2 / (3 (256 h)^2)) [L1] are far below 0.001 for these h
    for img, norm, h in ((base, nlm.NORM_L2, 0.05), (widen_u16(base), nlm.NORM_L1, 0.001)):
        table, _ = nlm.weight_table(img.dtype, h * (256 if img.dtype == np.uint16 else 1), norm, 7, 21)
        assert table[0] > 0 and not table[1:].any()
        assert np.array_equal(nlm.denoise(img, h, 7, 21), img)


def test_output_stays_inside_the_search_neighbourhood_range(gold):
    z, _ = gold
    from scipy import ndimage
    for img in (z["frame_odd"], widen_u16(z["frame_even"])):
        out = nlm.denoise(img, 10, 3, 9)
        for c in range(3):
            lo = ndimage.minimum_filter(img[..., c], size=9, mode="mirror")      # scipy's "mirror" is reflect-101
            hi = ndimage.maximum_filter(img[..., c], size=9, mode="mirror")
            assert np.all(out[..., c] >= lo) and np.all(out[..., c] <= hi)


def test_noise_falls_on_a_smooth_frame():
    y, x = np.mgrid[:48, :64]
    clean = np.rint(120 + 50 * np.sin(x / 11.0) * np.cos(y / 9.0)).astype(np.int64)[:, :, None] + np.array([10, 0, -10])
    noisy = np.clip(clean + hash_noise(clean.shape, 11, 8), 0, 255).astype(np.uint8)
    for img, scale in ((noisy, 1), (widen_u16(noisy), 256)):
        out = nlm.denoise(img, 10, 7, 21)
        before = np.mean((img.astype(np.float64) / scale - clean) ** 2)
        after = np.mean((out.astype(np.float64) / scale - clean) ** 2)
        assert after < before, (before, after)


def test_package_table_builder_equals_the_restatement():
    """weight_table of shinestacker_amd/denoise.py (chunked, stops at the first zero) against the restatement's whole table,
    every strength the stack action can pass (1-10), both dtypes, template = the amount and the default 7"""
    dn = importlib.import_module("shinestacker_amd.denoise")     # the package attribute of that name is the function
    for dt, norm, k in ((np.uint8, nlm.NORM_L2, 1), (np.uint16, nlm.NORM_L1, 256)):
        for h in range(1, 11):
            for tpl in (h, 7):
                full, shift = nlm.weight_table(dt, h * k, norm, tpl, 21)
                table, shift2 = dn.weight_table(dt, h * k, tpl, 21)
                cut = nlm.first_zero(full)
                assert shift == shift2 and table.dtype == np.uint32 and table.size == cut, (dt, h, tpl)
                assert np.array_equal(table, full[:cut]) and not full[cut:].any()
    full, _ = nlm.weight_table(np.uint8, 2.5, nlm.NORM_L2, 7, 21)
    assert np.array_equal(dn.weight_table(np.uint8, 2.5, 7, 21)[0], full[:nlm.first_zero(full)])


def test_python_argument_checks():
    from shinestacker_amd import BitDepthError, InvalidOptionError, denoise
    from shinestacker_amd.errors import BitDepthError as B2
    assert BitDepthError is B2
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(BitDepthError):
        denoise(img.astype(np.float32), 3)
    for bad_h in (0, -1):
        with pytest.raises(InvalidOptionError):
            denoise(img, bad_h)
    for tpl, srch in ((13, 21), (7, 23), (0, 21), (7.5, 21)):
        with pytest.raises(InvalidOptionError):
            denoise(img, 3, tpl, srch)
    with pytest.raises(InvalidOptionError):
        denoise(img[..., 0], 3)


class _Stacker:
    """stands in for the stacking algorithm: returns a fixed frame"""
    process = None
    do_step_callback = False

    def __init__(self, frame):
        self.frame = frame

    def focus_stack(self, files):
        return self.frame.copy()

    def steps_per_frame(self):
        return 1

    def name(self):
        return "stub"


def test_stack_action_option(tmp_path, monkeypatch):
    """A non-integral amount is refused when the action is built; amount 0 writes the stacker's frame untouched and imports
    nothing new; a positive amount calls denoise(stacked, amount, amount) after the message, before the file is written."""
    import sys
    from shinestacker_amd import FocusStack, FocusStackBunch, InvalidOptionError, StackJob, actions
    from shinestacker_amd.imageio import read_img
    frame = (hash_noise((24, 32, 3), 2, 100) + 128).astype(np.uint8)
    for cls in (FocusStack, FocusStackBunch):
        with pytest.raises(InvalidOptionError):
            cls("s", _Stacker(frame), denoise_amount=2.5)
        with pytest.raises(InvalidOptionError):
            cls("s", _Stacker(frame), denoise_amount=12)     # a template window of 13 is outside the kernel's range
    FocusStack("s", _Stacker(frame), denoise_amount=3.0)
    work = str(tmp_path)
    os.makedirs(os.path.join(work, "input"))
    for n in ("a.tif", "b.tif"):
        open(os.path.join(work, "input", n), "wb").close()

    def run(**kw):
        trace = []
        job = StackJob("job", work, input_path="input")
        action = FocusStack("s", _Stacker(frame), output_path="out", prefix="p_", **kw)
        action.sub_message_r = lambda msg, *a, **k: trace.append(msg)
        job.add_action(action)
        job.run()
        return read_img(os.path.join(work, "out", "p_a.tif")), trace
    seen = []
    dn = importlib.import_module("shinestacker_amd.denoise")
    monkeypatch.setattr(dn, "denoise", lambda img, *a, **k: seen.append(a) or img)
    out, trace = run()
    assert np.array_equal(out, frame) and seen == [] and not any("denoise" in m for m in trace)
    out, trace = run(denoise_amount=3.0)
    assert seen == [(3.0, 3)] and isinstance(seen[0][1], int)
    assert trace.index(": denoise image") == trace.index(": reading input files") + 1
    assert "denoise" in sys.modules["shinestacker_amd"].__all__ and actions is not None


def test_pipeline_refuses_a_non_integral_amount_before_touching_the_device():
    from shinestacker_amd import InvalidOptionError
    from shinestacker_amd.pipeline import align_and_stack, align_and_stack_device, bunches_then_stack
    with pytest.raises(InvalidOptionError):
        align_and_stack([np.zeros((64, 64, 3), np.uint8)], denoise_amount=2.5)
    with pytest.raises(InvalidOptionError):
        align_and_stack_device(0, 1, 64, 64, np.uint8, denoise_amount=-1)
    with pytest.raises(InvalidOptionError):
        bunches_then_stack(lambda i: None, 4, 64, 64, np.uint8, denoise_amount=0.5)
    with pytest.raises(InvalidOptionError):      # a template window of 13: refused before the stack is computed, not after
        align_and_stack([np.zeros((64, 64, 3), np.uint8)], denoise_amount=12)


def test_argument_validation_without_gpu(hiplib):
    """mi_nlm_denoise / mi_nlm_denoise_device refuse bad arguments before any device call"""
    lib = hiplib.load()
    table = np.array([19096, 100, 1], np.uint32)
    img = np.zeros((8, 8, 3), np.uint8)
    out = np.zeros_like(img)
    tp, ip, op = table.ctypes.data, img.ctypes.data, out.ctypes.data
    ok = (8, 8, hiplib.MI_U8, tp, 3, 6, 7, 21)
    assert lib.mi_nlm_denoise(0, None, op, *ok) == hiplib.MI_ERR_INVALID and b"null" in lib.mi_last_error()
    assert lib.mi_nlm_denoise(0, ip, op, 8, 8, hiplib.MI_U8, None, 3, 6, 7, 21) == hiplib.MI_ERR_INVALID
    assert lib.mi_nlm_denoise(0, ip, op, 8, 8, hiplib.MI_F32, tp, 3, 6, 7, 21) == hiplib.MI_ERR_INVALID
    assert lib.mi_nlm_denoise(0, ip, op, 0, 8, hiplib.MI_U8, tp, 3, 6, 7, 21) == hiplib.MI_ERR_INVALID
    assert lib.mi_nlm_denoise(0, ip, op, 8, 8, hiplib.MI_U8, tp, 0, 6, 7, 21) == hiplib.MI_ERR_INVALID
    assert lib.mi_nlm_denoise(0, ip, op, 8, 8, hiplib.MI_U8, tp, 3, 5, 7, 21) == hiplib.MI_ERR_INVALID     # shift of template 7 is 6
    assert b"shift" in lib.mi_last_error()
    assert lib.mi_nlm_denoise(0, ip, op, 8, 8, hiplib.MI_U8, tp, 3, 6, 0, 21) == hiplib.MI_ERR_INVALID
    assert lib.mi_nlm_denoise(0, ip, op, 8, 8, hiplib.MI_U8, tp, 3, 8, 13, 21) == hiplib.MI_ERR_UNSUPPORTED
    assert lib.mi_nlm_denoise(0, ip, op, 8, 8, hiplib.MI_U8, tp, 3, 6, 7, 23) == hiplib.MI_ERR_UNSUPPORTED
    zero = np.zeros(3, np.uint32)
    assert lib.mi_nlm_denoise(0, ip, op, 8, 8, hiplib.MI_U8, zero.ctypes.data, 3, 6, 7, 21) == hiplib.MI_ERR_INVALID
    # the device entry point: src == dst is refused (every output reads a neighbourhood of inputs)
    assert lib.mi_nlm_denoise_device(0, ip, ip, *ok, None) == hiplib.MI_ERR_INVALID and b"differ" in lib.mi_last_error()
    assert lib.mi_nlm_denoise_device(0, ip, None, *ok, None) == hiplib.MI_ERR_INVALID
    for name in ("mi_nlm_denoise", "mi_nlm_denoise_device"):
        assert name in hiplib.SIGNATURES and hasattr(C.CDLL(hiplib.LIB_PATH), name)


@pytest.mark.skipif(os.environ.get("MI_EXPECT_GPU") == "1", reason="GPU box")
def test_no_gpu_means_device_error(hiplib):
    if hiplib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    from shinestacker_amd import DeviceError, denoise
    with pytest.raises(DeviceError):
        denoise(np.zeros((8, 8, 3), np.uint8), 3)
