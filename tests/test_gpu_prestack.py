"""GPU: the Vignetting, MaskNoise and NoiseDetection kernels (csrc/kernels_prestack.hpp) and their actions against
tests/golden/prestack.{npz,json}, recorded from the reference's own classes by tools/gen_golden_prestack.py."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(hiplib):
    hiplib.require_device()
    with open(os.path.join(GOLDEN, "prestack.json")) as fh:
        meta = json.load(fh)
    return load_golden("prestack"), meta


def widen_u16(img8):
    """the uint16 frame of a recorded uint8 frame, as tools/gen_golden_prestack.py derives it (integers only)"""
    a = img8.astype(np.uint32)
    idx = np.arange(a.size, dtype=np.uint32).reshape(a.shape)
    return ((a << 8) | ((a * 37 + idx * 101) & 255)).astype(np.uint16)


def case_frame(z, c):
    fr = z["frame_" + c["frame"]]
    return widen_u16(fr) if c["u16"] else fr


def test_radial_ring_sums_equal_the_reference_means(gold):
    """Ring means identical (float64 array_equal, NaN positions included) for every recorded case: odd and even sizes,
    8- and 16-bit, sub-sampling 1 / 2 / 3 / 8, area and strided."""
    from shinestacker_amd import vignetting as vg
    z, meta = gold
    for c in meta["vignetting"]:
        radii, means = vg.radial_mean_intensity(case_frame(z, c), c["r_steps"], c["subsample"], c["fast_subsampling"])
        want = z[f"v_{c['name']}_means"]
        assert np.array_equal(radii, z[f"v_{c['name']}_radii"]), c["name"]
        assert np.array_equal(np.isnan(means), np.isnan(want)), c["name"]
        assert np.array_equal(means, want, equal_nan=True), (c["name"], np.nanmax(np.abs(means - want)))


def test_radial_ring_sums_full_size_against_the_rule_in_numpy(hiplib):
    """One 4000 x 6000 frame, no sub-sampling, against the rule as tests/prestack_restatement.py states it: integer BGR2GRAY,
    d in float64, radii[i] <= d < radii[i + 1] by binary search in the table; every pixel with d < r_max is counted once."""
    from shinestacker_amd import vignetting as vg
    h, w, r_steps = 4000, 6000, 100
    idx = np.arange(h * w * 3, dtype=np.uint32)
    idx ^= idx >> np.uint32(15)
    idx *= np.uint32(0x2c1b3c6d)
    idx ^= idx >> np.uint32(12)
    img = (idx >> np.uint32(8)).astype(np.uint8).reshape(h, w, 3)
    del idx
    buf = hiplib.DeviceBuffer(img.nbytes)
    buf.upload(img)
    _, means, sums, counts = vg.radial_ring_sums_device(buf.ptr, h, w, np.uint8, r_steps, subsample=1)
    buf.free()
    import prestack_restatement as pr
    assert np.array_equal(pr.ring_table(h, w, r_steps), vg.ring_table(h, w, r_steps))
    want_sums, want_counts = pr.ring_sums(img, r_steps)     # asserts itself that the counted pixels are those with d < r_max
    assert int(counts.sum()) == int(want_counts.sum()) == h * w - 1       # the corner pixel (0, 0) has d == r_max
    assert np.array_equal(counts.astype(np.int64), want_counts)
    assert np.array_equal(sums.astype(np.int64), want_sums)
    assert np.array_equal(means, want_sums / want_counts)


def _apply_recorded(z, c):
    from shinestacker_amd import vignetting as vg
    return vg.correct_vignetting(case_frame(z, c), c["max_correction"], c["black_threshold"], None,
                                 z[f"v_{c['name']}_params"].copy(), float(z[f"v_{c['name']}_v0"]))


def test_vignette_apply_with_recorded_params_matches_the_recorded_frames(gold):
    """The fit is out of the comparison (recorded parameters and v0 go in).  Bound: at most 1 count on at most 0.1 % of
    the values, the project's bound for float paths whose exp cannot be made bit-identical; with float64 throughout the
    expected number of differing values is zero -- it is printed, and a share above 1e-5 would mean something other than
    exp differs.  Pixels under the black threshold and pixels whose gain is 1 must be exactly the input."""
    from shinestacker_amd import vignetting as vg
    z, meta = gold
    n_cases = 0
    for c in meta["vignetting"]:
        if not c["has_out"]:
            continue
        n_cases += 1
        img, want = case_frame(z, c), z[f"v_{c['name']}_out"]
        got = _apply_recorded(z, c)
        assert got.shape == img.shape and (got != img).sum() > 0.5 * c["changed_values"]
        keep = np.concatenate([np.arange(a, b) for a, b in zip(c["out_rows"][::2], c["out_rows"][1::2])])   # the recorded rows
        img, got = img[keep], got[keep]
        assert got.dtype == want.dtype and got.shape == want.shape
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        share = float((diff != 0).mean())
        print(f"{c['name']}: {int((diff != 0).sum())} of {diff.size} values differ (share {share:.2e}), max {int(diff.max())}; "
              f"{int((got != img).sum())} values changed by the correction")
        assert diff.max() <= 1 and share <= 1e-3, c["name"]
        assert share <= 1e-5, (c["name"], "more than an exp ulp differs")
        threshold = c["black_threshold"] * (256 if c["u16"] else 1)
        black = img.min(axis=2) < threshold
        assert black.any() or c["frame"] == "a"
        assert np.array_equal(got[black], img[black]), c["name"]
        # gain == 1: the model is at (or, after the clip, above) its centre value
        h, w = case_frame(z, c).shape[:2]
        y, x = np.ogrid[:h, :w]
        r = np.sqrt((x - w / 2)**2 + (y - h / 2)**2)
        gain = np.clip(vg.sigmoid_model(r, *z[f"v_{c['name']}_params"]) / z[f"v_{c['name']}_v0"], 1e-6, 1)
        one = (gain == 1)[keep]
        assert np.array_equal(got[one], img[one]), c["name"]
    assert n_cases >= 4


class _Proc:
    id, name, working_path, plot_path = 0, "prestack", ".", "plots"
    filenames = ["0", "1", "2"]

    def __init__(self):
        self.messages = []

    def callback(self, *_a):
        return True

    def sub_message_r(self, *_a, **_k):
        pass

    def sub_message(self, msg, level=0, **_k):
        self.messages.append((level, msg))


def test_vignetting_run_frame_end_to_end(gold, monkeypatch):
    """run_frame with the LOCAL fit == the apply kernel fed those same parameters; `corrections` filled for that frame
    only; the frame comes back untouched when the fit fails."""
    from shinestacker_amd import Vignetting
    from shinestacker_amd import vignetting as vg
    z, meta = gold
    for c in meta["vignetting"]:
        if c["name"] not in ("a_u8_s8", "b_u8_s2_mc06", "c_u16_s1_mc06"):
            continue
        img = case_frame(z, c)
        action = Vignetting(r_steps=c["r_steps"], max_correction=c["max_correction"], black_threshold=c["black_threshold"],
                            subsample=c["subsample"], fast_subsampling=c["fast_subsampling"])
        action.begin(_Proc())
        out = action.run_frame(1, 0, img)
        assert action.params is not None
        rel = np.abs(action.params - z[f"v_{c['name']}_params"]) / z[f"v_{c['name']}_params"]
        assert rel.max() <= 1e-6, (c["name"], rel)
        want = vg.correct_vignetting(img, c["max_correction"], c["black_threshold"], None, action.params.copy(), action.v0)
        assert np.array_equal(out, want), c["name"]
        assert (out != img).any()
        for k, row in enumerate(action.corrections):
            assert np.isnan(row[0]) and np.isnan(row[2]) and np.isfinite(row[1])
            assert abs(row[1] - z[f"v_{c['name']}_percentile_radii"][k]) <= 1e-5 * abs(row[1]) + 1e-6
        action.end()
    import scipy.optimize

    def boom(*_a, **_k):
        raise RuntimeError("no fit")
    monkeypatch.setattr(scipy.optimize, "curve_fit", boom)
    action = Vignetting()
    proc = _Proc()
    action.begin(proc)
    img = z["frame_a"]
    out = action.run_frame(0, 0, img)
    assert out is img and all(np.isnan(r).all() for r in action.corrections)
    assert any("could not find vignetting model" in m for _, m in proc.messages)
    action.end()


def _mask_noise_input(z, meta, wide):
    img = widen_u16(z["mn_frame"]) if wide else z["mn_frame"].copy()
    if wide:
        for y0, y1, x0, x1, ch in meta["mask_noise_zeroed"]:
            if ch < 0:
                img[y0:y1, x0:x1] = 0
            else:
                img[y0:y1, x0:x1, ch] = 0
    return img


def test_mask_noise_equals_the_reference(gold):
    """Every recorded case (8 / 16 bit, kernel 3 / 5, MEAN / MEDIAN; corners, adjacent hot pixels, zero-valued neighbours,
    an all-zero window): the values at the hot pixels are the reference's, every other pixel is the input's, in place and
    into a second buffer."""
    from shinestacker_amd import MaskNoise
    z, meta = gold
    coords = z["mn_coords"]
    hot = z["mn_mask"] > 0
    for c in meta["mask_noise"]:
        img = _mask_noise_input(z, meta, c["u16"])
        mn = MaskNoise(kernel_size=c["kernel_size"], method=c["method"])
        mn.process = _Proc()
        mn.set_mask(z["mn_mask"])
        out = mn.run_frame(0, 0, img)
        assert out.dtype == img.dtype
        assert np.array_equal(out[coords[:, 0], coords[:, 1]], z[f"mn_{c['name']}_values"]), c["name"]
        assert np.array_equal(out[~hot], img[~hot]), c["name"]
        assert (out[hot] != img[hot]).any()
        # a distinct output buffer gives the same frame and leaves the source alone
        from shinestacker_amd import _lib
        src, dst = _lib.DeviceBuffer(img.nbytes), _lib.DeviceBuffer(img.nbytes)
        src.upload(img)
        mn.run_frame_device(0, src.ptr, img.shape[0], img.shape[1], img.dtype, dev_dst=dst.ptr)
        _lib.check(_lib.load().mi_device_synchronize(0))
        assert np.array_equal(dst.download(img.shape, img.dtype), out)
        assert np.array_equal(src.download(img.shape, img.dtype), img)
        src.free()
        dst.free()
        mn.end()
    # no hot pixel at all: the frame passes through
    mn = MaskNoise()
    mn.set_mask(np.zeros_like(z["mn_mask"]))
    assert np.array_equal(mn.run_frame(0, 0, z["mn_frame"]), z["mn_frame"])


def _small_stack(oracle, n=5, h=192, w=256):
    """frames with a small known motion, a synthetic vignette and hot pixels"""
    from test_gpu_ecc import make_pair, similarity
    frames = []
    y, x = np.ogrid[:h, :w]
    r = np.sqrt((x - w / 2)**2 + (y - h / 2)**2) / np.sqrt((w / 2)**2 + (h / 2)**2)
    fall = (1.0 - 0.45 * r**2)[:, :, None]
    hot = [(0, 0), (17, 40), (17, 41), (100, 200), (h - 1, w - 1), (150, 3)]
    for f in range(n):
        d = f - n // 2
        T = similarity(0.1 * d, 1 + 3e-4 * d, 1.1 * d, -0.7 * d, (w - 1) / 2, (h - 1) / 2)
        ref, mov = make_pair(oracle, T, h=h, w=w, seed=11, noise=2.0)
        fr = np.clip((ref if d == 0 else mov) * fall + 8, 0, 255).astype(np.uint8)
        for yy, xx in hot:
            fr[yy, xx] = 255
        frames.append(fr)
    mask = np.zeros((h, w), np.uint8)
    for yy, xx in hot:
        mask[yy, xx] = 255
    return frames, mask, hot


def test_pipeline_options_equal_the_steps_one_at_a_time(hiplib, oracle):
    """align_and_stack_device(mask_noise=, vignetting=) on a resident stack == MaskNoise then Vignetting through the
    sub-action classes on every frame, then the existing pipeline; with both options None the result and the transforms
    are bit-equal to a call that does not name them."""
    from shinestacker_amd import MaskNoise, Vignetting
    from shinestacker_amd.pipeline import align_and_stack_device
    frames, mask, _ = _small_stack(oracle)
    n, (h, w) = len(frames), frames[0].shape[:2]
    fb = frames[0].nbytes
    vopts = dict(subsample=2, r_steps=60)

    def resident(fs):
        buf = hiplib.DeviceBuffer(fb * n)
        for i, f in enumerate(fs):
            buf.upload(f, i * fb)
        return buf
    kw = dict(alignment_config=dict(subsample=1), min_size=16, arith="exact")
    buf = resident(frames)
    info = {}
    out, ms, ccs = align_and_stack_device(buf.ptr, n, h, w, np.uint8, mask_noise=dict(noise_mask=mask, kernel_size=3),
                                          vignetting=vopts, info=info, **kw)
    buf.free()
    mn, vg = MaskNoise(kernel_size=3), Vignetting(**vopts)
    mn.set_mask(mask)
    vg.begin(_Proc(), counts=n)
    fixed = [vg.run_frame(i, n // 2, mn.run_frame(i, n // 2, f)) for i, f in enumerate(frames)]
    assert all((a != b).any() for a, b in zip(fixed, frames))
    buf = resident(fixed)
    out2, ms2, ccs2 = align_and_stack_device(buf.ptr, n, h, w, np.uint8, **kw)
    buf.free()
    assert np.array_equal(out, out2)
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(ms, ms2)) and ccs == ccs2
    assert np.array_equal(np.array(info["vignetting_corrections"]), np.array(vg.corrections))
    # nothing existing moved
    buf = resident(frames)
    a = align_and_stack_device(buf.ptr, n, h, w, np.uint8, **kw)
    b = align_and_stack_device(buf.ptr, n, h, w, np.uint8, mask_noise=None, vignetting=None, **kw)
    assert np.array_equal(buf.download((n,) + frames[0].shape, np.uint8), np.stack(frames))
    buf.free()
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a[1], b[1]))
    assert not np.array_equal(a[0], out)


def test_host_pipeline_options(hiplib, oracle):
    """align_and_stack(frames, mask_noise=, vignetting=) == the corrected frames through align_and_stack"""
    from shinestacker_amd import MaskNoise, Vignetting
    from shinestacker_amd.align import ecc_estimator
    from shinestacker_amd.pipeline import align_and_stack
    frames, mask, _ = _small_stack(oracle, n=3)
    kw = dict(estimator=ecc_estimator(), alignment_config=dict(subsample=1), min_size=16, arith="exact")
    out, _ = align_and_stack(frames, mask_noise=dict(noise_mask=mask), vignetting=dict(subsample=2), **kw)
    mn, vg = MaskNoise(), Vignetting(subsample=2)
    mn.set_mask(mask)
    vg.begin(_Proc(), counts=3)
    fixed = [vg.run_frame(i, 1, mn.run_frame(i, 1, f)) for i, f in enumerate(frames)]
    out2, _ = align_and_stack(fixed, **kw)
    assert np.array_equal(out, out2)


def test_project_chain_on_files(hiplib, tmp_path):
    """NoiseDetection -> CombinedActions[MaskNoise, Vignetting, AlignFrames, BalanceFrames] -> FocusStack on the six img_jpg_crop frames with
    a synthetic vignette and hot pixels applied here; NoiseDetection writes the mask from six dark frames with the same hot pixels.
    Runs, writes the reference's file names, the hot pixels are gone from the aligned frames and their corner-to-centre
    intensity ratio is closer to 1 than the input's.  The frames are registered neighbour to neighbour (step_process) with
    a low correlation floor: these six frames differ in focus, which is not what this test is about."""
    from shinestacker_amd import (AlignFrames, BalanceFrames, CombinedActions, FocusStack, MaskNoise, NoiseDetection, PyramidStack,
                                  StackJob, Vignetting)
    from shinestacker_amd.noise_detection import read_mask
    from shinestacker_amd.align import ecc_estimator
    from shinestacker_amd.imageio import read_img, write_img
    work = str(tmp_path)
    os.makedirs(os.path.join(work, "in"))
    names = sorted(os.listdir(os.path.join(GOLDEN, "img_jpg_crop")))
    first = read_img(os.path.join(GOLDEN, "img_jpg_crop", names[0]))
    h, w = first.shape[:2]
    y, x = np.ogrid[:h, :w]
    r = np.sqrt((x - w / 2)**2 + (y - h / 2)**2) / np.sqrt((w / 2)**2 + (h / 2)**2)
    fall = (1.0 / (1.0 + np.exp(np.exp(6.0 * (r - 0.8)))) * (1 + np.exp(np.exp(-4.8))))[:, :, None]
    hot = [(5, 7), (h // 2, w // 2), (h // 2, w // 2 + 1), (h - 3, w - 9), (40, w - 2)]
    mask = np.zeros((h, w), np.uint8)
    for yy, xx in hot:
        mask[yy, xx] = 255
    # the mask comes from NoiseDetection over six dark frames (low hash noise, the same hot pixels)
    os.makedirs(os.path.join(work, "dark"))
    for f in range(6):
        idx = (np.arange(h * w * 3, dtype=np.uint32) + np.uint32(977 * f)) * np.uint32(0x9e3779b1)
        dark = ((idx >> np.uint32(13)) % np.uint32(7)).astype(np.uint8).reshape(h, w, 3)
        for yy, xx in hot:
            dark[yy, xx] = (50, 50, 50)     # far enough over the thresholds, low enough for the neighbours' blur to stay under
        write_img(os.path.join(work, "dark", f"d{f}.png"), dark)

    def ratio(img):
        g = img.astype(np.float64).mean(axis=2)
        ch, cw = h // 8, w // 8
        corners = np.mean([g[:ch, :cw].mean(), g[:ch, -cw:].mean(), g[-ch:, :cw].mean(), g[-ch:, -cw:].mean()])
        return corners / g[h // 2 - ch:h // 2 + ch, w // 2 - cw:w // 2 + cw].mean()
    in_ratio, bad_frames = [], []
    for n in names:
        img = read_img(os.path.join(GOLDEN, "img_jpg_crop", n))
        bad = np.clip(img * fall, 0, 255).astype(np.uint8)
        for yy, xx in hot:
            bad[yy, xx] = (255, 255, 255)
        in_ratio.append(ratio(bad))
        bad_frames.append(bad)
        write_img(os.path.join(work, "in", n), bad)
    job = StackJob("job", work, input_path="in")
    job.add_action(NoiseDetection("noise-map", input_path="dark"))
    job.add_action(CombinedActions("align", [MaskNoise(), Vignetting(subsample=2), AlignFrames(estimator=ecc_estimator(min_correlation=0.2), subsample=1),
                                             BalanceFrames(subsample=1)], input_path="in", output_path="aligned", step_process=True))
    job.add_action(FocusStack("stack", PyramidStack(), input_path="aligned", output_path="stack"))
    job.run()
    assert sorted(os.listdir(os.path.join(work, "aligned"))) == names
    assert np.array_equal(read_mask(os.path.join(work, "noise-map", "hot_pixels.png")), mask)    # NoiseDetection found exactly the planted pixels
    out = os.listdir(os.path.join(work, "stack"))
    assert len(out) == 1
    assert read_img(os.path.join(work, "stack", out[0])).shape == first.shape
    ref_idx = len(names) // 2

    for i, n in enumerate(names):
        al = read_img(os.path.join(work, "aligned", n))
        got = ratio(al)
        print(n, "corner / centre: vignetted", round(in_ratio[i], 4), "corrected", round(got, 4))
        assert abs(got - 1) < abs(in_ratio[i] - 1), n
    # The reference frame is neither warped nor balanced, so its aligned file is exactly Vignetting(MaskNoise(input)); MaskNoise
    # put the truncated mean of the non-zero 3 x 3 values at every hot pixel (stated here in NumPy), which is far below the
    # planted 255; and the file differs at the hot pixels from what the chain would have written without MaskNoise.
    bad = bad_frames[ref_idx]
    al = read_img(os.path.join(work, "aligned", names[ref_idx]))
    masked = bad.copy()
    for yy, xx in hot:
        for ch in range(3):
            win = bad[max(0, yy - 1):yy + 2, max(0, xx - 1):xx + 2, ch].astype(np.int64).reshape(-1)
            masked[yy, xx, ch] = win[win != 0].sum() // (win != 0).sum()
        print("hot pixel", (yy, xx), "planted", bad[yy, xx], "masked", masked[yy, xx])
        assert (masked[yy, xx] < bad[yy, xx]).all()
    mn = MaskNoise()
    mn.set_mask(mask)
    assert np.array_equal(mn.run_frame(ref_idx, ref_idx, bad), masked)
    vg = Vignetting(subsample=2)
    vg.begin(_Proc(), counts=len(names))
    assert np.array_equal(al, vg.run_frame(ref_idx, ref_idx, masked))
    without = vg.run_frame(ref_idx, ref_idx, bad)
    # (at a far corner both may saturate after the gain, so this is asked of the hot pixels together, not of each)
    assert any((al[yy, xx] != without[yy, xx]).any() for yy, xx in hot)


def test_noise_detection_equals_the_reference(gold, tmp_path):
    """Mean image, hot map and the four counts identical to the recording for every case (all frames, the max_frames
    quirk at 1 and 3, blur 3 with unequal thresholds, blur 7); the PNG written and read back is the map; MaskNoise.begin
    reads it and finds the same pixels."""
    from shinestacker_amd import MaskNoise, NoiseDetection, StackJob
    from shinestacker_amd.imageio import write_img
    from shinestacker_amd.noise_detection import read_mask
    z, meta = gold
    assert len(meta["noise_detection"]) >= 5
    for c in meta["noise_detection"]:
        work = tmp_path / c["name"]
        os.makedirs(work / "frames")
        for f, fr in enumerate(z["nd_frames"]):
            write_img(str(work / "frames" / f"f{f:03d}.png"), fr)
        trace = []
        cbs = {k: (lambda *a, k=k: trace.append([k, *a[2:]]) or True) for k in ("step_counts", "after_step", "check_running")}
        job = StackJob("job", str(work), input_path="frames", callbacks=cbs)
        action = NoiseDetection("noise-map", **c["options"])
        job.add_action(action)
        action.run_core()
        want_mean = z[f"nd_{c['name']}_mean"] if f"nd_{c['name']}_mean" in z else z["nd_all_mean"]
        assert trace == c["trace"], c["name"]
        assert np.array_equal(action.mean_img, want_mean), c["name"]
        assert np.array_equal(action.hot_rgb, z[f"nd_{c['name']}_map"]), c["name"]
        assert action.hot_counts == c["counts"], (c["name"], action.hot_counts)
        path = work / "noise-map" / "hot_pixels.png"
        assert c["file_name"] == "noise-map/hot_pixels.png" and np.array_equal(read_mask(str(path)), action.hot_rgb)
        mn = MaskNoise()
        mn.begin(job)
        assert np.array_equal(mn._coords, np.argwhere(z[f"nd_{c['name']}_map"] > 0))
        assert np.array_equal(mn.run_frame(0, 0, z["nd_frames"][0])[action.hot_rgb == 0], z["nd_frames"][0][action.hot_rgb == 0])
    # a frame size that is not a multiple of four elements, more frames than one batch
    odd = [np.full((5, 7, 3), 10 + f, np.uint8) for f in range(11)]
    work = tmp_path / "odd"
    os.makedirs(work / "frames")
    for f, fr in enumerate(odd):
        write_img(str(work / "frames" / f"f{f:03d}.png"), fr)
    job = StackJob("job", str(work), input_path="frames")
    action = NoiseDetection("noise-map")
    job.add_action(action)
    action.run_core()
    assert np.array_equal(action.mean_img, np.full((5, 7, 3), 15, np.uint8)) and action.hot_counts == [0, 0, 0, 0]
