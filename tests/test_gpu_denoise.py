"""GPU: the post-stack denoise kernel (csrc/kernels_denoise.hpp) behind denoise(), denoise_device(), the stack actions'
denoise_amount and the pipeline's denoise_amount= -- every comparison is array_equal against tests/golden/denoise.{npz,json}
(recorded from the reference's own wrapper, tools/gen_golden_denoise.py) or against the NumPy restatement."""
import json
import os

import numpy as np
import pytest

import nlm_restatement as nlm
from conftest import GOLDEN, load_golden
from test_denoise_host import case_args, case_frame, hash_noise, widen_u16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(hiplib):
    hiplib.require_device()
    with open(os.path.join(GOLDEN, "denoise.json")) as fh:
        return load_golden("denoise"), json.load(fh)


def test_denoise_equals_every_recorded_case(gold):
    """both dtypes; odd and even frame sizes; frames smaller than the 32 x 32 tile (20 x 24, 3 x 2) and narrower than the
    search window (40 x 7: reflect-101 applied more than once); template 1 / 3 / 5 / 7 / 11 and the even 4 / 10; search
    5 / 21 and the even 6 / 20; h 1 / 3 / 10 and a non-integral one.  What the fixtures reach of the kernel: template half
    sizes 0, 1, 2, 3 and 5 (not 4; on uint16, 2 only on the 20 x 24 partial tile), search half sizes 2, 3 and 10, the table in LDS for every
    uint8 case and read from global memory only for uint16 at h 10.  test_gpu_poststack_edges.py runs the rest: every template
    half size, search half sizes 0, 1, 5 and 10, both table placements for both dtypes, one-row / one-column / one-pixel
    frames, frames on the tile grid, saturated frames."""
    from shinestacker_amd import denoise
    z, meta = gold
    seen = set()
    for c in meta["cases"]:
        img = case_frame(z, c)
        out = denoise(img, *case_args(c))
        want = z["out_" + c["name"]]
        assert out.dtype == img.dtype and out.shape == img.shape
        assert np.array_equal(out, want), (c["name"], int((out != want).sum()))
        seen.add((c["cv2_call"]["template"], c["cv2_call"]["search"], c["h_luminance"]))
    assert {t for t, _, _ in seen} >= {1, 3, 5, 7, 11} and {s for _, s, _ in seen} >= {5, 21} and {h for _, _, h in seen} >= {1, 3, 10}
    for amount in (1, 3, 4):
        assert np.array_equal(denoise(z["frame_small"], amount, amount), z[f"stack_amount{amount}"])


def big_frame(h, w, wide):
    """smooth texture + integer hash noise, built row block by row block to bound the host memory"""
    out = np.empty((h, w, 3), np.uint16 if wide else np.uint8)
    x = np.arange(w)[None, :]
    for y0 in range(0, h, 512):
        y = np.arange(y0, min(h, y0 + 512))[:, None]
        tex = np.rint(120 + 60 * np.sin(x / 37.0) * np.cos(y / 29.0) + 30 * ((x // 500 + y // 400) % 2)).astype(np.int64)
        blk = tex[:, :, None] + np.array([12, 0, -12]) + hash_noise((y.shape[0], w, 3), y0 + 1, 6)
        blk = np.clip(blk, 0, 255).astype(np.uint8)
        out[y0:y0 + y.shape[0]] = widen_u16(blk) if wide else blk
    return out


@pytest.mark.parametrize("h,w,wide", [(4000, 6000, False), (5760, 8640, True)])
def test_full_size_frame_windows_equal_the_restatement(hiplib, h, w, wide):
    """Six 64 x 64 windows -- four corners, an edge, the centre -- of a full-size frame against the restatement run on the
    window plus its 13-pixel halo (search 21 / 2 + template 7 / 2), cut from the frame: at the frame's own border the
    restatement reflects as the kernel must, at a cut the 13 outer pixels of its result are discarded."""
    from shinestacker_amd.denoise import denoise_device
    img = big_frame(h, w, wide)
    src, dst = hiplib.DeviceBuffer(img.nbytes), hiplib.DeviceBuffer(img.nbytes)
    try:
        src.upload(img)
        denoise_device(src.ptr, dst.ptr, h, w, img.dtype, 3)
        out = dst.download(img.shape, img.dtype)
    finally:
        src.free()
        dst.free()
    halo, n = 13, 64
    windows = [(0, 0), (0, w - n), (h - n, 0), (h - n, w - n), (h // 2 - 7, 0), (h // 2 - 31, w // 2 - 33), (0, w // 3 + 5)]
    changed = 0
    for y0, x0 in windows:
        ya, yb, xa, xb = max(0, y0 - halo), min(h, y0 + n + halo), max(0, x0 - halo), min(w, x0 + n + halo)
        want = nlm.denoise(img[ya:yb, xa:xb], 3)[y0 - ya:y0 - ya + n, x0 - xa:x0 - xa + n]
        got = out[y0:y0 + n, x0:x0 + n]
        assert np.array_equal(got, want), ((y0, x0), int((got != want).sum()))
        changed += int((got != img[y0:y0 + n, x0:x0 + n]).sum())
    assert changed > 0


def test_host_and_device_entry_points_agree_and_aliasing_is_refused(hiplib, gold):
    from shinestacker_amd import denoise
    from shinestacker_amd.denoise import denoise_device
    z, _ = gold
    for img in (z["frame_odd"], widen_u16(z["frame_even"])):
        h, w = img.shape[:2]
        src, dst = hiplib.DeviceBuffer(img.nbytes), hiplib.DeviceBuffer(img.nbytes)
        try:
            src.upload(img)
            denoise_device(src.ptr, dst.ptr, h, w, img.dtype, 3, 5, 21)
            assert dst.download(img.shape, img.dtype).tobytes() == denoise(img, 3, 5, 21).tobytes()
            assert np.array_equal(src.download(img.shape, img.dtype), img)
            with pytest.raises(ValueError):
                denoise_device(src.ptr, src.ptr, h, w, img.dtype, 3, 5, 21)
        finally:
            src.free()
            dst.free()


def _png_inputs(work):
    from shinestacker_amd.imageio import read_img, write_img
    os.makedirs(os.path.join(work, "input"))
    for n in sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop"))):
        write_img(os.path.join(work, "input", os.path.splitext(n)[0] + ".png"), read_img(os.path.join(GOLDEN, "img_jpg_crop", n)))


def test_focus_stack_with_denoise_amount(hiplib, tmp_path):
    """FocusStack(denoise_amount=3) on the img_jpg_crop frames (as PNG, so the written files are the arrays): the file equals
    the restatement applied to the file the same action writes with denoise_amount=0, with the amount as strength and as
    template size; ': denoise image' follows the stacker's messages and precedes the write."""
    from shinestacker_amd import FocusStack, PyramidStack, StackJob
    from shinestacker_amd.imageio import read_img
    hiplib.require_device()
    work = str(tmp_path)
    _png_inputs(work)
    traces = {}
    for amount in (0, 3):
        trace = traces.setdefault(amount, [])
        job = StackJob("job", work, input_path="input")
        action = FocusStack("s", PyramidStack(), output_path=f"out{amount}", denoise_amount=amount)
        real = action.sub_message_r
        action.sub_message_r = lambda msg, *a, _t=trace, _r=real, **k: (_t.append(msg), _r(msg, *a, **k))[1]
        job.add_action(action)
        job.run()
    (name,) = os.listdir(os.path.join(work, "out0"))
    plain, den = read_img(os.path.join(work, "out0", name)), read_img(os.path.join(work, "out3", name))
    assert np.array_equal(den, nlm.denoise(plain, 3, 3)) and not np.array_equal(den, plain)
    assert traces[3][-1] == ": denoise image" and traces[3][:-1] == traces[0] and traces[0][0] == ": reading input files"


def test_pipeline_denoise_amount(hiplib, tmp_path):
    """align_and_stack(..., denoise_amount=3) == denoise(align_and_stack(...), 3, 3); the same for the resident entry point,
    downloaded and written to out_dev, and for bunches_then_stack"""
    from shinestacker_amd import denoise
    from shinestacker_amd.imageio import read_img
    from shinestacker_amd.pipeline import align_and_stack, align_and_stack_device, bunches_then_stack
    hiplib.require_device()
    names = sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop")))
    frames = [read_img(os.path.join(GOLDEN, "img_jpg_crop", n)) for n in names]
    h, w = frames[0].shape[:2]

    def est(i0, i1, fc, mc, ac):
        return 500, np.array([[1.0, 0.0, 0.25], [0.0, 1.0, -0.5]])
    kw = dict(estimator=est, alignment_config={'subsample': 1})
    plain, _ = align_and_stack(frames, **kw)
    den, _ = align_and_stack(frames, denoise_amount=3, **kw)
    assert np.array_equal(den, denoise(plain, 3, 3)) and not np.array_equal(den, plain)

    buf = hiplib.DeviceBuffer(frames[0].nbytes * len(frames))
    out_dev = hiplib.DeviceBuffer(frames[0].nbytes)
    try:
        buf.upload(np.stack(frames))
        plain = align_and_stack_device(buf.ptr, len(frames), h, w, np.uint8)[0]
        den = align_and_stack_device(buf.ptr, len(frames), h, w, np.uint8, denoise_amount=3)[0]
        assert np.array_equal(den, denoise(plain, 3, 3))
        assert align_and_stack_device(buf.ptr, len(frames), h, w, np.uint8, denoise_amount=3, out_dev=out_dev.ptr)[0] is None
        assert np.array_equal(out_dev.download(frames[0].shape, np.uint8), den)
    finally:
        buf.free()
        out_dev.free()
    plain, _ = bunches_then_stack(lambda i: frames[i], len(frames), h, w, np.uint8, frames=3, overlap=1)
    den, _ = bunches_then_stack(lambda i: frames[i], len(frames), h, w, np.uint8, frames=3, overlap=1, denoise_amount=3)
    assert np.array_equal(den, denoise(plain, 3, 3))
