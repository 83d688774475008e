"""CPU: tests/prestack_restatement.py against the reference's recordings in tests/golden/prestack.{npz,json}.  The GPU tests
in test_gpu_prestack_edges.py compare the kernels with that restatement at shapes nothing was recorded at; this file is what
stands behind the restatement there."""
import json
import os

import numpy as np
import pytest

import prestack_restatement as pr
from conftest import GOLDEN, load_golden


@pytest.fixture(scope="module")
def gold():
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


def test_ring_sums_give_the_recorded_means(gold):
    z, meta = gold
    assert len(meta["vignetting"]) >= 15
    for c in meta["vignetting"]:
        img = case_frame(z, c)
        sums, counts = pr.ring_sums(img, c["r_steps"], c["subsample"], c["fast_subsampling"])
        assert sums.dtype == counts.dtype == np.int64 and sums.shape == counts.shape == (c["r_steps"],)
        assert list(pr.subsampled_gray(img, c["subsample"], c["fast_subsampling"]).shape) == c["sub_shape"], c["name"]
        means, want = pr.ring_means(sums, counts), z[f"v_{c['name']}_means"]
        assert np.array_equal(np.isnan(means), np.isnan(want)), c["name"]
        assert np.array_equal(means, want, equal_nan=True), c["name"]


def test_vignette_gives_the_recorded_frames(gold):
    """Bound as in test_gpu_prestack.py: at most 1 count, on a share of at most 1e-5 of the values (the recording's exp is
    rounded once from long double, NumPy's need not be); black pixels are exactly the input."""
    z, meta = gold
    n_cases = 0
    for c in meta["vignetting"]:
        if not c["has_out"]:
            continue
        n_cases += 1
        img, want = case_frame(z, c), z[f"v_{c['name']}_out"]
        got = pr.vignette(img, *z[f"v_{c['name']}_params"], float(z[f"v_{c['name']}_v0"]), c["max_correction"], c["black_threshold"])
        keep = np.concatenate([np.arange(a, b) for a, b in zip(c["out_rows"][::2], c["out_rows"][1::2])])
        img, got = img[keep], got[keep]
        assert got.dtype == want.dtype and got.shape == want.shape
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        share = float((diff != 0).mean())
        print(f"{c['name']}: {int((diff != 0).sum())} of {diff.size} values differ (share {share:.2e}), max {int(diff.max())}")
        assert diff.max() <= 1 and share <= 1e-5, c["name"]
        assert (got != img).sum() > 0.1 * got.size, c["name"]
        black = img.min(axis=2) < c["black_threshold"] * (256 if c["u16"] else 1)
        assert black.any() or c["frame"] == "a"
        assert np.array_equal(got[black], img[black]), c["name"]
        # row blocks of the restatement are the rows of the whole frame
        a, b = c["out_rows"][0], c["out_rows"][1]
        part = pr.vignette(case_frame(z, c)[a:b], *z[f"v_{c['name']}_params"], float(z[f"v_{c['name']}_v0"]), c["max_correction"],
                           c["black_threshold"], rows=(a, b), height=case_frame(z, c).shape[0])
        assert np.array_equal(part, got[:b - a]), c["name"]
    assert n_cases >= 4


def _mask_noise_input(z, meta, wide):
    img = widen_u16(z["mn_frame"]) if wide else z["mn_frame"].copy()
    if wide:
        for y0, y1, x0, x1, ch in meta["mask_noise_zeroed"]:
            if ch < 0:
                img[y0:y1, x0:x1] = 0
            else:
                img[y0:y1, x0:x1, ch] = 0
    return img


def test_mask_noise_gives_the_recorded_values(gold):
    z, meta = gold
    coords, hot = z["mn_coords"], z["mn_mask"] > 0
    assert len(meta["mask_noise"]) == 8
    for c in meta["mask_noise"]:
        img = _mask_noise_input(z, meta, c["u16"])
        src = img.copy()
        out = pr.mask_noise(img, coords, c["kernel_size"], c["method"])
        assert np.array_equal(img, src) and out.dtype == img.dtype
        assert np.array_equal(out[coords[:, 0], coords[:, 1]], z[f"mn_{c['name']}_values"]), c["name"]
        assert np.array_equal(out[~hot], img[~hot]), c["name"]
        assert (out[hot] != img[hot]).any()


def test_accumulate_and_hot_map_give_the_recorded_maps(gold):
    z, meta = gold
    assert [c["name"] for c in meta["noise_detection"]] == ["all", "max1", "max3", "blur3_th", "blur7"]
    for c in meta["noise_detection"]:
        n = c["frames_averaged"]
        sums = pr.accumulate(z["nd_frames"][:n])
        assert sums.dtype == np.uint32 and sums.shape == z["nd_frames"][0].shape
        opts = c["options"]
        mean, hot, counts = pr.hot_map(sums, n, opts.get("blur_size", 5), opts.get("channel_thresholds", [13, 13, 13]))
        want_mean = z[f"nd_{c['name']}_mean"] if f"nd_{c['name']}_mean" in z else z["nd_all_mean"]
        assert mean.dtype == np.uint8 and np.array_equal(mean, want_mean), c["name"]
        assert hot.dtype == np.uint8 and np.array_equal(hot, z[f"nd_{c['name']}_map"]), c["name"]
        assert counts == c["counts"], (c["name"], counts)
        assert counts[0] > 0


def test_reflect101_mirrors_as_often_as_it_takes():
    assert list(pr.reflect101(np.arange(-3, 8), 5)) == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert list(pr.reflect101(np.arange(-3, 5), 2)) == [1, 0, 1, 0, 1, 0, 1, 0]
    assert list(pr.reflect101(np.arange(-3, 6), 3)) == [1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert list(pr.reflect101(np.arange(-3, 4), 1)) == [0] * 7
