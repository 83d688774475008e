"""GPU: the retouch filters -- the unsharp kernel (csrc/kernels_unsharp.hpp) behind unsharp_mask() / unsharp_mask_device(), the
white balance through the per-channel look-up kernel, and the pipeline's white_balance= / unsharp= -- every comparison is
array_equal against tests/golden/retouch.{npz,json} (recorded from the reference's own modules, tools/gen_golden_retouch.py)
or against the NumPy restatement."""
import json
import os

import numpy as np
import pytest

import unsharp_restatement as usr
from conftest import GOLDEN, load_golden
from test_denoise_host import hash_noise
from test_retouch_host import case_args, case_frame, widen_u16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(hiplib):
    hiplib.require_device()
    with open(os.path.join(GOLDEN, "retouch.json")) as fh:
        return load_golden("retouch"), json.load(fh)


def test_unsharp_mask_equals_every_recorded_case(gold):
    """both dtypes and both branches; odd and even frame sizes; frames smaller than the 32 x 32 tile (20 x 24, 3 x 2) and
    narrower than the halo (40 x 7 at radius 4: reflect-101 applied more than once); windows 1 to 33"""
    from shinestacker_amd import unsharp_mask
    z, meta = gold
    windows = set()
    for c in meta["unsharp"]:
        img = case_frame(z, c)
        out = unsharp_mask(img, *case_args(c))
        want = z["out_" + c["name"]]
        assert out.dtype == img.dtype and out.shape == img.shape
        assert np.array_equal(out, want), (c["name"], int((out != want).sum()))
        windows.add(c["cv2_calls"][0]["ksize"])
    assert windows >= {1, 3, 7, 9, 13, 17, 19, 25, 33}


def test_white_balance_equals_every_recorded_case(gold):
    from shinestacker_amd import white_balance_from_rgb
    z, meta = gold
    for c in meta["white_balance"]:
        img = case_frame(z, c)
        out = white_balance_from_rgb(img, c["target_rgb"])
        assert out.dtype == img.dtype and np.array_equal(out, z["wb_" + c["name"]]), c["name"]


def big_frame(h, w, wide):
    """smooth texture, checker blocks with hard edges and integer hash noise, built row block by row block"""
    out = np.empty((h, w, 3), np.uint16 if wide else np.uint8)
    x = np.arange(w)[None, :]
    for y0 in range(0, h, 512):
        y = np.arange(y0, min(h, y0 + 512))[:, None]
        tex = np.rint(120 + 60 * np.sin(x / 37.0) * np.cos(y / 29.0) + 70 * ((x // 50 + y // 40) % 2)).astype(np.int64)
        blk = tex[:, :, None] + np.array([12, 0, -12]) + hash_noise((y.shape[0], w, 3), y0 + 1, 6)
        blk = np.clip(blk, 0, 255).astype(np.uint8)
        out[y0:y0 + y.shape[0]] = widen_u16(blk) if wide else blk
    return out


@pytest.mark.parametrize("h,w,wide", [(4000, 6000, False), (5760, 8640, True)])
def test_full_size_frame_windows_equal_the_restatement(hiplib, h, w, wide):
    """Seven 64 x 64 windows -- four corners, an edge, the centre, and one across a tile seam off the 32-pixel grid -- of a
    full-size frame at radius 1 and radius 4, both branches, against the restatement run on the window plus its halo of
    ksize / 2 pixels cut from the frame: at the frame's own border the restatement reflects as the kernel must, at a cut the
    outer halo of its result is discarded."""
    from shinestacker_amd.sharpen import unsharp_mask_device, window_size
    img = big_frame(h, w, wide)
    n = 64
    windows = [(0, 0), (0, w - n), (h - n, 0), (h - n, w - n), (h // 2 - 7, 0), (h // 2 - 31, w // 2 - 33), (1011, w // 3 + 5)]
    src, dst = hiplib.DeviceBuffer(img.nbytes), hiplib.DeviceBuffer(img.nbytes)
    try:
        src.upload(img)
        for radius, amount, threshold in ((1, 0.5, 0), (4, 1.5, 0), (4, 1.5, 10), (1, 3.0, 10)):
            unsharp_mask_device(src.ptr, dst.ptr, h, w, img.dtype, radius, amount, threshold)
            hiplib.check(hiplib.load().mi_device_synchronize(0))
            out = dst.download(img.shape, img.dtype)
            halo = window_size(img.dtype, radius) // 2
            changed = 0
            for y0, x0 in windows:
                ya, yb, xa, xb = max(0, y0 - halo), min(h, y0 + n + halo), max(0, x0 - halo), min(w, x0 + n + halo)
                want = usr.unsharp_mask(img[ya:yb, xa:xb], radius, amount, threshold)[y0 - ya:y0 - ya + n, x0 - xa:x0 - xa + n]
                got = out[y0:y0 + n, x0:x0 + n]
                assert np.array_equal(got, want), ((radius, amount, threshold), (y0, x0), int((got != want).sum()))
                changed += int((got != img[y0:y0 + n, x0:x0 + n]).sum())
            assert changed > 0
    finally:
        src.free()
        dst.free()


def test_host_and_device_entry_points_agree_and_aliasing_is_refused(hiplib, gold):
    from shinestacker_amd import unsharp_mask, white_balance_from_rgb
    from shinestacker_amd.sharpen import unsharp_mask_device
    from shinestacker_amd.white_balance import white_balance_device
    z, _ = gold
    for img in (z["frame_odd"], widen_u16(z["frame_even"])):
        h, w = img.shape[:2]
        src, dst = hiplib.DeviceBuffer(img.nbytes), hiplib.DeviceBuffer(img.nbytes)
        try:
            src.upload(img)
            for args in ((2, 1.5, 0), (3, 0.5, 10)):
                unsharp_mask_device(src.ptr, dst.ptr, h, w, img.dtype, *args)
                hiplib.check(hiplib.load().mi_device_synchronize(0))
                assert dst.download(img.shape, img.dtype).tobytes() == unsharp_mask(img, *args).tobytes()
            assert np.array_equal(src.download(img.shape, img.dtype), img)
            with pytest.raises(ValueError):
                unsharp_mask_device(src.ptr, src.ptr, h, w, img.dtype, 2, 1.5, 0)
            want = white_balance_from_rgb(img, (246, 233, 178))
            white_balance_device(src.ptr, dst.ptr, h * w, img.dtype, (246, 233, 178))
            assert np.array_equal(dst.download(img.shape, img.dtype), want)
            white_balance_device(src.ptr, src.ptr, h * w, img.dtype, (246, 233, 178))      # in place is allowed here
            assert np.array_equal(src.download(img.shape, img.dtype), want)
        finally:
            src.free()
            dst.free()


def test_pipeline_retouch_options(hiplib):
    """align_and_stack(..., denoise_amount=d, white_balance=t, unsharp=u) == unsharp(white_balance(denoise(plain))); with both
    new arguments None the result is today's; the same for the resident entry point (downloaded and written to out_dev)
    and for bunches_then_stack; every subset of the three filters keeps the order"""
    from shinestacker_amd import denoise, unsharp_mask, white_balance_from_rgb
    from shinestacker_amd.imageio import read_img
    from shinestacker_amd.pipeline import align_and_stack, align_and_stack_device, bunches_then_stack
    hiplib.require_device()
    names = sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop")))
    frames = [read_img(os.path.join(GOLDEN, "img_jpg_crop", n)) for n in names]
    h, w = frames[0].shape[:2]
    t, u = (246, 233, 178), (2.0, 1.5, 0)

    def est(i0, i1, fc, mc, ac):
        return 500, np.array([[1.0, 0.0, 0.25], [0.0, 1.0, -0.5]])
    kw = dict(estimator=est, alignment_config={'subsample': 1})
    plain, _ = align_and_stack(frames, **kw)
    again, _ = align_and_stack(frames, white_balance=None, unsharp=None, **kw)
    assert np.array_equal(again, plain)
    full, _ = align_and_stack(frames, denoise_amount=3, white_balance=t, unsharp=u, **kw)
    assert np.array_equal(full, unsharp_mask(white_balance_from_rgb(denoise(plain, 3, 3), t), *u))
    assert not np.array_equal(full, plain)
    assert np.array_equal(align_and_stack(frames, white_balance=t, **kw)[0], white_balance_from_rgb(plain, t))
    u2 = (1.0, 0.5, 10)
    assert np.array_equal(align_and_stack(frames, unsharp=u2, **kw)[0], unsharp_mask(plain, *u2))
    assert np.array_equal(align_and_stack(frames, white_balance=t, unsharp=u2, **kw)[0],
                          unsharp_mask(white_balance_from_rgb(plain, t), *u2))
    assert np.array_equal(align_and_stack(frames, denoise_amount=3, white_balance=t, **kw)[0],
                          white_balance_from_rgb(denoise(plain, 3, 3), t))

    buf = hiplib.DeviceBuffer(frames[0].nbytes * len(frames))
    out_dev = hiplib.DeviceBuffer(frames[0].nbytes)
    try:
        buf.upload(np.stack(frames))
        plain = align_and_stack_device(buf.ptr, len(frames), h, w, np.uint8)[0]
        want = unsharp_mask(white_balance_from_rgb(denoise(plain, 3, 3), t), *u)
        got = align_and_stack_device(buf.ptr, len(frames), h, w, np.uint8, denoise_amount=3, white_balance=t, unsharp=u)[0]
        assert np.array_equal(got, want)
        assert align_and_stack_device(buf.ptr, len(frames), h, w, np.uint8, denoise_amount=3, white_balance=t, unsharp=u,
                                      out_dev=out_dev.ptr)[0] is None
        assert np.array_equal(out_dev.download(frames[0].shape, np.uint8), want)
        assert align_and_stack_device(buf.ptr, len(frames), h, w, np.uint8, white_balance=t, out_dev=out_dev.ptr)[0] is None
        assert np.array_equal(out_dev.download(frames[0].shape, np.uint8), white_balance_from_rgb(plain, t))
    finally:
        buf.free()
        out_dev.free()
    plain, _ = bunches_then_stack(lambda i: frames[i], len(frames), h, w, np.uint8, frames=3, overlap=1)
    got, _ = bunches_then_stack(lambda i: frames[i], len(frames), h, w, np.uint8, frames=3, overlap=1, denoise_amount=3,
                                white_balance=t, unsharp=u)
    assert np.array_equal(got, unsharp_mask(white_balance_from_rgb(denoise(plain, 3, 3), t), *u))
