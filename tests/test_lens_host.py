"""CPU: the lens cases of lens_cases.py mean something -- the restatement has the properties the kernel is meant to have, no
case is vacuous, the masks take both values where they should, autoscale removes every replicated border -- and the host side
of lens.py (Lens, its constructors, LensCorrection, the pipeline's option) validates and builds what it says."""
import ctypes
import inspect

import numpy as np
import pytest

import lens_cases as LC
import lens_restatement as R
from shinestacker_amd import InvalidOptionError, Lens, LensCorrection, lens, pipeline

MOVING = ("barrel", "pincushion", "outward", "CA", "mixed")


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_identity_plane_comes_out_as_it_went_in(dtype):
    """(1, 0, 0, 0) is a copy for any centre -- also far outside the frame and at non-representable positions -- on every
    plane of the identity lens and on the green plane of the CA lens"""
    for shape in LC.SHAPES:
        h, w = shape
        f = LC.frame("random", shape, dtype)
        for c in (None, (0.3 * (w - 1), 0.8 * (h - 1)), (-1234.567, 9876.543), (w / 3.0, h / 7.0), (1e6 + 0.1, -1e6 - 0.3)):
            out, mask = R.remap(f, LC.LENSES["identity"], c, return_mask=True)
            assert np.array_equal(out, f) and mask.all(), (shape, c)
            assert np.array_equal(R.remap(f, LC.LENSES["CA"], c)[:, :, 1], f[:, :, 1]), (shape, c)


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_saturated_frame_stays_saturated(dtype):
    for shape in LC.SHAPES:
        for name in LC.LENSES:
            for kind in LC.CENTRES:
                out, _ = LC.reference(name, kind, "saturated", shape, dtype)
                assert (out == LC.maxv(dtype)).all(), (shape, name, kind)


def test_largest_sum_fits_32_bits():
    assert 65535 * 1024 + 512 < 2 ** 31


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_no_case_is_vacuous(dtype):
    """on every shape of at least 15 pixels each moving lens changes at least 25 % of the pixels of a random frame"""
    lowest = 1.0
    for shape in LC.SHAPES:
        if shape[0] * shape[1] < 15:
            continue
        f = LC.frame("random", shape, dtype)
        for name in MOVING:
            for kind in LC.CENTRES:
                out, _ = LC.reference(name, kind, "random", shape, dtype)
                changed = (out != f).any(axis=2).mean()
                print(f"{np.dtype(dtype).name} {shape} {name} {kind}: {changed:.3f}")
                lowest = min(lowest, changed)
                assert changed >= 0.25, (shape, name, kind, changed)
    print("lowest share of changed pixels:", lowest)


@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_collapse_reads_the_centre_and_zoom_out_clamps(dtype):
    shape = (33, 47)
    f = LC.frame("random", shape, dtype)
    out, mask = LC.reference("collapse", "default", "random", shape, dtype)
    assert (out == f[16, 23]).all() and mask.all()         # the centre (23, 16) is a pixel
    out, mask = LC.reference("zoom-out", "default", "random", shape, dtype)
    assert (mask == 0).mean() > 0.8                          # almost everything clamps
    assert np.array_equal(out[0, 0], f[0, 0]) and np.array_equal(out[-1, -1], f[-1, -1])


def test_masks_take_both_values():
    for name in ("outward", "CA", "zoom-out"):
        for kind in LC.CENTRES:
            _, mask = LC.reference(name, kind, "random", (33, 47), np.uint8)
            assert set(np.unique(mask)) == {0, 1}, (name, kind)
    for name in ("identity", "barrel", "collapse"):
        _, mask = LC.reference(name, "default", "random", (33, 47), np.uint8)
        assert mask.all(), name


def test_autoscale_leaves_no_replicated_border():
    """scaled(autoscale(h, w)) keeps every source position inside the frame: an all-ones mask"""
    n = 0
    for shape in LC.SHAPES:
        h, w = shape
        if h < 3 or w < 5:
            continue
        for name in ("barrel", "outward", "CA"):
            for kind in LC.CENTRES:
                L = LC.lens_of(name, kind, shape)
                f = L.autoscale(h, w)
                assert np.isfinite(f) and f > 0
                S = L.scaled(f)
                assert np.array_equal(S.coefficients(), R.scaled(LC.LENSES[name], f).reshape(12))
                _, mask = R.remap(LC.frame("random", shape, np.uint8), S.coefficients().reshape(3, 4), LC.centre(kind, shape), True)
                assert mask.all(), (shape, name, kind, f)
                n += 1
    assert n == 2 * 3 * 12
    # it is the LARGEST such factor: a little more and the outward lens leaves the frame again
    L = LC.lens_of("outward", "default", (33, 47))
    f = L.autoscale(33, 47)
    assert f < 1.0
    _, mask = R.remap(LC.frame("random", (33, 47), np.uint8), R.scaled(LC.LENSES["outward"], f * 1.01), None, True)
    assert not mask.all()
    # a lens that keeps inside the frame is magnified up to the border
    assert LC.lens_of("barrel", "default", (33, 47)).autoscale(33, 47) > 1.0
    assert Lens((0, 0, 0, 0)).autoscale(33, 47) == 1.0       # nothing constrains the collapse
    assert Lens().autoscale(1, 1) == 1.0
    for bad in ((-0.5, 3), (47, 3), (3, 33.5), (3, -1e-9)):
        with pytest.raises(InvalidOptionError):
            Lens(LC.LENSES["barrel"], bad).autoscale(33, 47)
    with pytest.raises(InvalidOptionError):
        Lens().autoscale(0, 5)


def test_inv_r2_and_struct_state_the_restatement():
    for shape in LC.SHAPES:
        h, w = shape
        for kind in LC.CENTRES:
            c = LC.centre(kind, shape)
            cx, cy = R.default_centre(h, w) if c is None else c
            assert lens.inv_r2(h, w, cx, cy) == float(R.inv_r2(h, w, cx, cy))
            s = LC.lens_of("CA", kind, shape).struct(h, w)
            assert (s.cx, s.cy) == (cx, cy)
            assert list(s.k) == [float(v) for p in LC.LENSES["CA"] for v in p]
    assert lens.inv_r2(1, 1, 0.0, 0.0) == 0.0
    assert ctypes.sizeof(Lens().struct(3, 3)) == 112


def test_lens_constructors():
    assert Lens().k == ((1.0, 0.0, 0.0, 0.0),) * 3 and Lens().centre is None
    assert Lens((1, -0.1, 0.02, 0)).k == ((1.0, -0.1, 0.02, 0.0),) * 3
    three = ((0.97, 0.02, 0, 0), (1, 0, 0, 0), (1.03, -0.01, 0, 0))
    assert Lens(three).k == tuple(tuple(float(v) for v in p) for p in three)
    assert Lens(np.array(three)).k == Lens(three).k and Lens(np.array([1, 2, 3, 4.0])).k == ((1.0, 2.0, 3.0, 4.0),) * 3
    assert Lens(three, centre=(3, 4.5)).centre == (3.0, 4.5)
    assert Lens.distortion(-0.12, 0.02) == Lens((1, -0.12, 0.02, 0))
    assert Lens.distortion(0.08, -0.03, 0.01, k0=0.93, centre=(1, 2)) == Lens((0.93, 0.08, -0.03, 0.01), (1, 2))
    ca = Lens.chromatic(red=(1.03, -0.01), blue=(0.97, 0.02, 0, 0))
    assert ca == Lens(three) and ca.k[1] == (1.0, 0.0, 0.0, 0.0)
    assert Lens.chromatic() == Lens()
    # the DNG opcode: planes in R, G, B order, kr0..kr3 with or without the (zero) tangential terms
    r, g, b = (1.03, -0.01, 0, 0), (1, 0, 0, 0), (0.97, 0.02, 0, 0)
    assert Lens.from_warp_rectilinear([r, g, b]) == Lens(three)
    assert Lens.from_warp_rectilinear([r + (0, 0), g + (0.0, 0.0), b + (0, 0)]) == Lens(three)
    assert Lens.from_warp_rectilinear((1, -0.12, 0.02, 0)) == Lens.distortion(-0.12, 0.02)
    assert Lens.from_warp_rectilinear([(1, -0.12, 0.02, 0, 0, 0)]) == Lens.distortion(-0.12, 0.02)
    assert Lens(three).scaled(0.5).k[2] == (1.03 * 0.5, -0.01 * 0.5, 0.0, 0.0)
    assert Lens(three, (1, 2)).scaled(2).centre == (1.0, 2.0)
    assert Lens(three).resolved_centre(33, 47) == (23.0, 16.0) and Lens(three).resolved_centre(2, 2) == (0.5, 0.5)


@pytest.mark.parametrize("make", [Lens, lambda *a, **k: LensCorrection(*a, **k)], ids=["Lens", "LensCorrection"])
def test_validation(make):
    """LensCorrection refuses what Lens refuses"""
    nan, inf = float("nan"), float("inf")
    for bad in (None, 1.0, "barrel", (1, 0, 0), (1, 0, 0, 0, 0), (1, nan, 0, 0), (1, 0, inf, 0), (1, 0, 0, "x"), (1, 0, 0, True),
                ((1, 0, 0, 0), (1, 0, 0, 0)), ((1, 0, 0, 0),) * 4, ((1, 0, 0, 0), (1, 0, 0), (1, 0, 0, 0)),
                ((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, -inf, 0))):
        with pytest.raises(InvalidOptionError):
            make(bad)
    make((1, 0, 0, 0))
    make(((1, 0, 0, 0),) * 3)


def test_validation_of_the_rest():
    nan = float("nan")
    for bad in (3, (1,), (1, 2, 3), (nan, 1), ("a", 1), (True, 1), (2.0 ** 30 + 1, 0), (0, -1e300)):
        with pytest.raises(InvalidOptionError):
            Lens(centre=bad)
    for bad in ((), (1, 0, 0, 0, 0), (1, nan), "x"):
        with pytest.raises(InvalidOptionError):
            Lens.chromatic(red=bad)
        with pytest.raises(InvalidOptionError):
            Lens.chromatic(blue=bad)
    for bad in (None, (), (1, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 1e-3, 0), (1, 0, 0, 0, 0, -2), [(1, 0, 0, 0)] * 2,
                [(1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0, 0, 0.5)], [(1, 0, 0, 0), (1, 0, 0), (1, 0, 0, 0)], (1, nan, 0, 0)):
        with pytest.raises(InvalidOptionError):
            Lens.from_warp_rectilinear(bad)
    for bad in (nan, float("inf"), "2", None, True, 1e308):
        with pytest.raises(InvalidOptionError):
            Lens((9, 9, 9, 9)).scaled(bad)
    with pytest.raises(InvalidOptionError):
        LensCorrection(Lens(), autoscale="yes")
    for bad in ({"autoscale": True}, {"lens": Lens(), "scale": 2}, {"lens": (1, 0, 0)}, (1, 0, 0)):
        with pytest.raises(InvalidOptionError):
            lens.make_step(bad)
    step = lens.make_step({"lens": (1, 0.1, 0, 0), "autoscale": True}, device=3)
    assert step.autoscale and step.device == 3 and step.lens == Lens.distortion(0.1)
    assert step.lens_for(33, 47) == step.lens.scaled(step.lens.autoscale(33, 47))
    assert lens.make_step(Lens()).lens_for(33, 47) == Lens()
    # frames are refused before anything touches a device
    f = np.zeros((4, 5, 3), np.uint8)
    for bad in (f[:, :, 0], np.zeros((4, 5, 4), np.uint8), np.zeros((0, 5, 3), np.uint8)):
        with pytest.raises(InvalidOptionError):
            lens.correct(bad, Lens())
    from shinestacker_amd import BitDepthError
    with pytest.raises(BitDepthError):
        lens.correct(f.astype(np.float32), Lens())
    with pytest.raises(InvalidOptionError):
        lens.correct(f, (1, 0, 0))
    Lens(centre=(2.0 ** 30, -2.0 ** 30))
    # a caller's scratch frame that does not hold the frame is refused before a kernel is queued that would write past it
    from shinestacker_amd import Cfa, demosaic

    class Small:
        ptr, nbytes = 4096, 4 * 6 * 3 - 1
    with pytest.raises(InvalidOptionError, match="lens_scratch"):
        demosaic.debayer_device(4096, 8192, 4, 6, np.uint8, Cfa(), lens=Lens(), lens_scratch=Small())
    with pytest.raises(InvalidOptionError, match="lens_scratch"):
        demosaic.debayer_device(4096, 8192, 4, 6, np.uint16, Cfa(), lens=Lens(), lens_scratch=object())


def test_lens_none_leaves_the_prestack_steps_as_they_were():
    assert pipeline._prestack_steps(None, None, 5, 0) == []
    assert pipeline._prestack_steps(None, None, 5, 0, None) == []
    assert pipeline._prestack_steps(None, None, 5, 0, lens=None) == []
    mask = np.zeros((4, 6), np.uint8)
    steps = pipeline._prestack_steps({"noise_mask": mask}, {"r_steps": 10}, 5, 0)
    assert [type(s).__name__ for s in steps] == ["MaskNoise", "Vignetting"]
    # the lens correction comes last: behind MaskNoise and Vignetting, ahead of the estimate and the warp
    steps = pipeline._prestack_steps({"noise_mask": mask}, {"r_steps": 10}, 5, 0, Lens.distortion(-0.1))
    assert [type(s).__name__ for s in steps] == ["MaskNoise", "Vignetting", "LensCorrection"]
    assert steps[-1].lens == Lens.distortion(-0.1) and not hasattr(steps[-1], "corrections")
    steps = pipeline._prestack_steps(None, None, 5, 0, {"lens": Lens.distortion(0.1), "autoscale": True})
    assert [type(s).__name__ for s in steps] == ["LensCorrection"] and steps[0].autoscale
    for s in steps:
        s.end()                                             # nothing was allocated: nothing to free, no device needed
    with pytest.raises(InvalidOptionError):
        pipeline._prestack_steps(None, None, 5, 0, (1, 0, 0))
    for fn in (pipeline.align_and_stack, pipeline.align_and_stack_device):
        assert inspect.signature(fn).parameters["lens"].default is None
    from shinestacker_amd import demosaic
    for fn in (demosaic.debayer, demosaic.debayer_device, demosaic.debayer_frames_device):
        assert inspect.signature(fn).parameters["lens"].default is None


def test_img_ref_passes_the_reference_through_the_lens_correction(tmp_path, monkeypatch):
    """CombinedActions.img_ref -- where AlignFrames gets its reference -- applies the sub-actions that correct the frame's
    geometry, and only those, and only where the reference is an input file (not step_process: there it is an output file)"""
    import os
    from shinestacker_amd import AlignFrames, CombinedActions, MaskNoise, actions
    from shinestacker_amd.imageio import write_img
    frame = LC.frame("random", (8, 9), np.uint8)
    for d in ("in", "out"):
        os.makedirs(tmp_path / d)
        write_img(str(tmp_path / d / "a.png"), frame)
    step = LensCorrection(Lens.distortion(-0.1))
    seen = []
    monkeypatch.setattr(step, "run_frame", lambda idx, ref, img: seen.append((idx, ref)) or img + 1)
    mn = MaskNoise()
    monkeypatch.setattr(mn, "run_frame", lambda *a: pytest.fail("MaskNoise leaves the reference as the reference does"))
    assert step.corrects_reference and not getattr(mn, "corrects_reference", False)
    for step_process, want in ((False, frame + 1), (True, frame)):
        job = CombinedActions("lens", [mn, step, AlignFrames()], input_path="in", output_path="out", step_process=step_process)
        job.input_full_path, job.output_dir, job.filenames = str(tmp_path / "in"), str(tmp_path / "out"), ["a.png"]
        assert np.array_equal(job.img_ref(0), want), step_process
    assert seen == [(0, 0)]
    step.enabled = False
    job = CombinedActions("lens", [step], input_path="in", output_path="out")
    job.input_full_path, job.output_dir, job.filenames = str(tmp_path / "in"), str(tmp_path / "out"), ["a.png"]
    assert np.array_equal(job.img_ref(0), frame)


def test_lens_correction_is_a_sub_action():
    from shinestacker_amd import CombinedActions, SubAction
    step = LensCorrection(Lens.distortion(-0.1))
    assert isinstance(step, SubAction) and step.enabled
    for name in ("begin", "run_frame", "run_frame_device", "end"):
        assert callable(getattr(step, name))
    job = CombinedActions("lens", [step], input_path="in", output_path="out")
    assert job._actions == [step]


def test_every_way_a_row_of_taps_is_loaded_occurs():
    shared = [n for n, k in LC.LENSES.items() if np.ndim(k) == 1]
    assert shared == ["identity", "barrel", "pincushion", "outward", "zoom-out", "collapse"]
    seen = {s: set() for s in LC.SHAPES}
    for shape in LC.SHAPES:
        for name in shared:
            for kind in LC.CENTRES:
                seen[shape] |= LC.tap_loads(name, kind, shape)
    assert seen[(1, 1)] == {"clamped", "last pixel"}                # a 3-byte image: nothing but bytes
    assert seen[(7, 1)] == {"clamped", "last pixel"}                # one column: never two neighbours
    for shape in LC.SHAPES[4:]:                                     # from 3 x 5 on every shape has all four
        assert seen[shape] == set(LC.TAP_LOADS), (shape, seen[shape])
    assert LC.tap_loads("barrel", "default", (33, 47)) == {"pair"}   # (it reads inside the frame, away from its end)
    assert LC.tap_loads("identity", "default", (33, 47)) == set(LC.TAP_LOADS)
    # 16 bits: a pair or the same pixel twice, nothing else
    for shape in LC.SHAPES[4:]:
        got = set().union(*(LC.tap_loads(n, k, shape, np.uint16) for n in shared for k in LC.CENTRES))
        assert got == {"pair", "clamped"}, (shape, got)
    assert LC.tap_loads("identity", "default", (7, 1), np.uint16) == {"clamped"}
    # planes with their own coordinates (8 bits): both ways of loading a row's two samples occur from 3 x 5 on
    for shape in LC.SHAPES[4:]:
        got = set().union(*(LC.sample_loads("CA", k, shape) for k in LC.CENTRES))    # (its red plane reads past the sides)
        assert got == set(LC.SAMPLE_LOADS), (shape, got)
        assert "dword" in LC.sample_loads("mixed", "default", shape)                # (mixed reads inside small frames)
    assert LC.sample_loads("CA", "default", (7, 1)) == {"apart"}


def test_overflowing_coefficients_are_defined():
    """inf and NaN on the way to the position end in [-1, w] x [-1, h]: the restatement warns of nothing and clamps"""
    import warnings
    for shape in ((33, 47), (16, 64)):
        f = LC.frame("random", shape, np.uint8)
        for k in LC.OVERFLOWING.values():
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                for c in range(3):
                    X, Y = R.positions(shape[0], shape[1], R.planes(k)[c], None)
                    assert X.min() >= -32 and X.max() <= 32 * shape[1] and Y.min() >= -32 and Y.max() <= 32 * shape[0]
                out, mask = R.remap(f, k, None, return_mask=True)
            assert not mask.all()
    # a NaN does occur: on the centre's column dx = 0 meets s = inf
    k0, k1, k2, k3 = LC.OVERFLOWING["huge"]
    with np.errstate(over="ignore", invalid="ignore"):
        u = np.float64(0.5)
        s = ((k3 * u + k2) * u + k1) * u + k0
        assert np.isinf(s) and np.isnan(np.float64(0.0) * s)
    assert "clamped" in LC.tap_loads("zoom-out", "default", (33, 47))


def test_the_case_table_is_the_issues():
    assert LC.SHAPES[:6] == [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (33, 47)]
    assert set(LC.EDGES) == {(h, w) for h in (15, 16, 17) for w in (63, 64, 65)}
    assert LC.SHAPES[-1][0] > 2 * LC.TILE_H and LC.SHAPES[-1][1] > 2 * LC.TILE_W      # three tiles by three
    assert max(h * w for h, w in LC.SHAPES) <= 256 * 1024
    assert list(LC.LENSES) == ["identity", "barrel", "pincushion", "outward", "CA", "mixed", "zoom-out", "collapse"]
    text = open(lens.__file__.replace("lens.py", "csrc/kernels_lens.hpp")).read()
    assert f"TILE_W = {LC.TILE_W}, TILE_H = {LC.TILE_H}" in text
