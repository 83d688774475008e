"""CPU: the host side of the Vignetting and MaskNoise mirrors against tests/golden/prestack.{npz,json}, which
tools/gen_golden_prestack.py recorded from the reference's own classes.  Nothing here needs a GPU: the fit, v0, the ring
table and the percentile radii are host code; the option checks and the exceptions come before any device call."""
import inspect
import json
import logging
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "prestack.json")) as fh:
        meta = json.load(fh)
    return load_golden("prestack"), meta


def test_signatures_and_defaults_are_the_references(gold):
    import shinestacker_amd as sa
    _, meta = gold
    for name, cls in (("Vignetting", sa.Vignetting), ("MaskNoise", sa.MaskNoise), ("NoiseDetection", sa.NoiseDetection)):
        sig = inspect.signature(cls.__init__).parameters
        ref = meta["signatures"][name]
        ref_pos = [p for p in ref if p["kind"] == "POSITIONAL_OR_KEYWORD"]
        mine = [k for k, v in sig.items() if v.kind == v.POSITIONAL_OR_KEYWORD][1:]
        assert mine[:len(ref_pos)] == [p["name"] for p in ref_pos], (name, mine)
        for p in ref_pos:
            v = sig[p["name"]]
            assert (v.default is not inspect.Parameter.empty) == p["has_default"], (name, p["name"])
            if p["has_default"]:
                assert repr(v.default) == p["default"], (name, p["name"])
        if any(p["kind"] == "VAR_KEYWORD" for p in ref):
            assert any(v.kind == v.VAR_KEYWORD for v in sig.values()), name
    from shinestacker_amd import constants, noise_detection, vignetting
    for k, v in meta["constants"].items():
        if k == "MAX_NOISY_PIXELS":
            assert noise_detection.MAX_NOISY_PIXELS == v
        elif k == "CLIP_EXP":
            assert vignetting.CLIP_EXP == v
        elif k == "VALID_INTERPOLATE":
            assert sorted(constants.VALID_INTERPOLATE) == v
        else:
            assert getattr(constants, k) == v, k
    vg = sa.Vignetting()
    assert (vg.r_steps, vg.black_threshold, vg.max_correction, vg.subsample, vg.fast_subsampling) == (100, 1.0, 1, 8, False)
    assert list(vg.percentiles) == [0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95]
    assert list(sa.Vignetting(percentiles=(0.9, 0.1)).percentiles) == [0.1, 0.9]       # np.sort, as the reference


def test_ring_table_v0_and_percentile_radii_equal_the_fixture(gold, hiplib):
    """These involve no fit: the table is np.linspace on the sub-sampled size (mi_subsampled_size), v0 is the model at 0,
    the percentile radii are fsolve from the RECORDED parameters.  Equal, not close: the mirror's model evaluates exp the way
    the fixture was recorded (float64 rounded once from long double), so nothing here depends on the NumPy build."""
    from shinestacker_amd import vignetting as vg
    z, meta = gold
    for c in meta["vignetting"]:
        fr = z["frame_" + c["frame"]]
        hs, ws = vg.subsampled_shape(fr.shape[0], fr.shape[1], c["subsample"], c["fast_subsampling"])
        assert [hs, ws] == c["sub_shape"], c["name"]
        table = vg.ring_table(hs, ws, c["r_steps"])
        assert np.array_equal(table, z[f"v_{c['name']}_table"]), c["name"]
        assert np.array_equal((table[1:] + table[:-1]) / 2, z[f"v_{c['name']}_radii"]), c["name"]
        params = z[f"v_{c['name']}_params"]
        v0 = vg.sigmoid_model(0, *params)
        assert v0 == z[f"v_{c['name']}_v0"], c["name"]
        got = np.array(vg.percentile_radii(params, v0, c["percentiles"]))
        assert np.array_equal(got, z[f"v_{c['name']}_percentile_radii"]), c["name"]


def test_ring_means_are_sum_over_count_with_nan_for_empty_rings():
    from shinestacker_amd.vignetting import ring_means
    m = ring_means(np.array([10, 0, 7], np.uint64), np.array([4, 0, 2], np.uint32))
    assert m[0] == 2.5 and np.isnan(m[1]) and m[2] == 3.5
    vals = np.array([3, 200, 41, 41, 7], np.uint8)
    assert ring_means([int(vals.sum())], [vals.size])[0] == np.mean(vals)


def test_local_fit_agrees_with_the_recorded_fit(gold):
    """From the recorded ring means, this machine's scipy finds the recorded parameters to a relative 1e-6 (curve_fit's
    default ftol 1e-8 with two decades of room: the recorded fit may come from another scipy build)."""
    from shinestacker_amd import vignetting as vg
    z, meta = gold
    worst = 0.0
    for c in meta["vignetting"]:
        p = vg.fit_sigmoid(z[f"v_{c['name']}_radii"], z[f"v_{c['name']}_means"])
        p[1] /= c["subsample"]
        p[2] *= c["subsample"]
        rel = np.abs(p - z[f"v_{c['name']}_params"]) / np.abs(z[f"v_{c['name']}_params"])
        worst = max(worst, rel.max())
        print(c["name"], "relative difference of (i0, k, r0):", rel)
        assert rel.max() <= 1e-6, (c["name"], rel)
    print("largest relative difference:", worst)


class _Proc:
    id, name, working_path, plot_path = 0, "prestack", ".", "plots"
    filenames = ["0.png", "1.png", "2.png"]

    def __init__(self):
        self.messages = []

    def callback(self, *_a):
        return True

    def sub_message_r(self, msg, **_k):
        pass

    def sub_message(self, msg, level=logging.INFO, **_k):
        self.messages.append((level, msg))


def test_fit_failure_leaves_the_frame_and_the_corrections_alone(gold, monkeypatch):
    """vignetting.py:126-135: when the fit raises, a warning is logged, the corrections stay NaN and the frame is returned
    as it came (here checked on the host half, `_fit`; the GPU test checks run_frame)."""
    from shinestacker_amd import vignetting as vg
    z, meta = gold
    c = meta["vignetting"][0]

    def boom(*_a, **_k):
        raise RuntimeError("Optimal parameters not found")
    import scipy.optimize
    monkeypatch.setattr(scipy.optimize, "curve_fit", boom)
    action = vg.Vignetting(r_steps=c["r_steps"])
    proc = _Proc()
    action.begin(proc)
    assert len(action.corrections) == 7 and all(a.shape == (3,) and np.isnan(a).all() for a in action.corrections)
    action.r_max = 1.0
    assert action._fit(1, z[f"v_{c['name']}_radii"], z[f"v_{c['name']}_means"]) is None
    assert action.params is None
    assert all(np.isnan(a).all() for a in action.corrections)
    assert any(level == logging.WARNING and "could not find vignetting model" in msg for level, msg in proc.messages)


def test_mask_noise_refuses_what_the_reference_refuses(tmp_path):
    from shinestacker_amd import ImageLoadError, InvalidOptionError, MaskNoise
    with pytest.raises(InvalidOptionError):
        MaskNoise(method="MODE")
    for ks in (0, 4, -3, 2.5):
        with pytest.raises(InvalidOptionError):
            MaskNoise(kernel_size=ks)
    proc = _Proc()
    proc.working_path = str(tmp_path)
    mn = MaskNoise()
    assert (mn.noise_mask, mn.kernel_size, mn.method, mn.ks2, mn.ks2_1) == ("noise-map/hot_pixels.png", 3, "MEAN", 1, 2)
    assert MaskNoise(noise_mask='').noise_mask == "noise-map/hot_pixels.png"
    with pytest.raises(ImageLoadError, match="file not found"):
        mn.begin(proc)
    os.makedirs(tmp_path / "noise-map")
    (tmp_path / "noise-map" / "hot_pixels.png").write_bytes(b"not a png")
    with pytest.raises(ImageLoadError, match="failed to load image file"):
        mn.begin(proc)
    # more than 1000 hot pixels: the reference's RuntimeError, with its text, when a frame arrives
    from PIL import Image
    mask = np.zeros((40, 50), np.uint8)
    mask.reshape(-1)[:1001] = 255
    Image.fromarray(mask).save(tmp_path / "noise-map" / "hot_pixels.png")
    mn.begin(proc)
    assert np.array_equal(mn.noise_mask_img, mask)
    with pytest.raises(RuntimeError, match="Noise map contains too many hot pixels: 1001"):
        mn.run_frame(0, 0, np.ones((40, 50, 3), np.uint8))


def test_mask_file_round_trip_keeps_coordinates(gold, tmp_path):
    """begin() reads an 8-bit gray PNG the way cv2.imread(IMREAD_GRAYSCALE) does; the hot pixels come out in np.argwhere order"""
    from PIL import Image
    from shinestacker_amd import MaskNoise
    z, _ = gold
    os.makedirs(tmp_path / "noise-map")
    Image.fromarray(z["mn_mask"]).save(tmp_path / "noise-map" / "hot_pixels.png")
    proc = _Proc()
    proc.working_path = str(tmp_path)
    mn = MaskNoise()
    mn.begin(proc)
    assert np.array_equal(mn.noise_mask_img, z["mn_mask"])
    assert np.array_equal(mn._coords, z["mn_coords"])


def test_pipeline_options_default_to_none():
    from shinestacker_amd import pipeline
    for fn in (pipeline.align_and_stack, pipeline.align_and_stack_device):
        sig = inspect.signature(fn).parameters
        assert sig["mask_noise"].default is None and sig["vignetting"].default is None


def _noise_job(tmp_path, frames, callbacks, **opts):
    from shinestacker_amd import NoiseDetection, StackJob
    from shinestacker_amd.imageio import write_img
    os.makedirs(tmp_path / "frames", exist_ok=True)
    for f, fr in enumerate(frames):
        write_img(str(tmp_path / "frames" / f"f{f:03d}.png"), fr)
    job = StackJob("job", str(tmp_path), input_path="frames", callbacks=callbacks)
    action = NoiseDetection("noise-map", **opts)
    job.add_action(action)
    return job, action


def _host_device_steps(monkeypatch):
    """the two device steps of NoiseDetection replaced by their NumPy statement, so that the host loop runs without a GPU"""
    from shinestacker_amd import NoiseDetection
    state = {}

    def add(self, frames):
        self._sum = None
        state["sum"] = state.get("sum", 0) + np.stack(frames).astype(np.uint32).sum(axis=0)

    def hot(self, counter, shape):
        mean = (state["sum"] // counter).astype(np.uint8)
        return mean, np.zeros(shape[:2], np.uint8), [0, 0, 0, 0]
    monkeypatch.setattr(NoiseDetection, "_device_add", add)
    monkeypatch.setattr(NoiseDetection, "_device_map", hot)
    return state


def test_noise_detection_callback_trace_and_max_frames_quirk(gold, tmp_path, monkeypatch):
    """step_counts announces min(n, max_frames) while max_frames + 1 frames are averaged (the reference's loop stops at
    i > max_frames): trace and mean image == the recording, for max_frames -1, 1 and 3."""
    from shinestacker_amd.noise_detection import read_mask
    z, meta = gold
    for c in meta["noise_detection"]:
        if c["name"] not in ("all", "max1", "max3"):
            continue
        state = _host_device_steps(monkeypatch)
        trace = []
        cbs = {k: (lambda *a, k=k: trace.append([k, *a[2:]]) or True) for k in ("step_counts", "after_step", "check_running")}
        job, action = _noise_job(tmp_path / c["name"], z["nd_frames"], cbs, **c["options"])
        action.run_core()
        assert trace == c["trace"], c["name"]
        assert np.array_equal(action.mean_img, z[f"nd_{c['name']}_mean"]), c["name"]
        assert state["sum"].max() <= 255 * c["frames_averaged"]
        assert read_mask(str(tmp_path / c["name"] / "noise-map" / "hot_pixels.png")).shape == action.mean_img.shape[:2]


def test_noise_detection_refuses_16_bit_and_stops_when_asked(gold, tmp_path, monkeypatch):
    from shinestacker_amd import BitDepthError, InvalidOptionError, NoiseDetection, RunStopException
    z, _ = gold
    _host_device_steps(monkeypatch)
    job, action = _noise_job(tmp_path / "wide", [z["nd_frames"][0].astype(np.uint16) * 257], None)
    with pytest.raises(BitDepthError):
        action.run_core()
    seen = []
    cbs = {"check_running": lambda *_a: bool(seen.append(1) or len(seen) < 2)}
    job, action = _noise_job(tmp_path / "stop", z["nd_frames"], cbs)
    with pytest.raises(RunStopException):
        action.run_core()
    assert len(seen) == 2
    with pytest.raises(InvalidOptionError):
        NoiseDetection(blur_size=9)
    nd = NoiseDetection(file_name='')
    assert (nd.file_name, nd.max_frames, nd.blur_size, list(nd.channel_thresholds)) == ("noise-map/hot_pixels.png", -1, 5, [13, 13, 13])


def test_frame_multi_directory_takes_one_folder_or_several(gold, tmp_path):
    from shinestacker_amd import NoiseDetection, StackJob
    from shinestacker_amd.imageio import write_img
    z, _ = gold
    for d, names in (("a", ["2.png", "1.png"]), ("b", ["3.png", "note.txt"])):
        os.makedirs(tmp_path / d)
        for n in names:
            if n.endswith(".png"):
                write_img(str(tmp_path / d / n), z["nd_frames"][0])
            else:
                (tmp_path / d / n).write_text("x")
    job = StackJob("job", str(tmp_path), input_path="a")
    one = NoiseDetection("n1")
    job.add_action(one)
    assert one.folder_filelist() == ["a/1.png", "a/2.png"] and one.folder_list_str() == "folder: a"
    many = NoiseDetection("n2", input_path=["a", "b"], reverse_order=True)
    job.add_action(many)
    assert many.folder_filelist() == ["a/2.png", "a/1.png", "b/3.png"] and many.folder_list_str() == "folders: a, b"
    assert NoiseDetection("n3", input_path=["a", "b"], resample=2).input_path == ["a", "b"]


def test_resident_vignetting_needs_frames_of_a_multiple_of_16_bytes():
    """mi_vignette_apply_device takes 16-byte aligned frames; a contiguous resident stack of 203 x 301 uint8 frames cannot
    give that to every frame, and the pipeline says so before anything touches the device."""
    from shinestacker_amd import InvalidOptionError
    from shinestacker_amd.pipeline import align_and_stack_device
    with pytest.raises(InvalidOptionError, match="multiple of 16"):
        align_and_stack_device(0x1000, 3, 203, 301, np.uint8, vignetting={})
