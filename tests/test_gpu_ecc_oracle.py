"""GPU: the ECC estimator (kernels_ecc.hpp, aligner_solve) against its float64 statement (oracle/ecc_oracle.py), step by
step and converged, across the entry points (ecc_similarity, Aligner.estimate_batch / estimate_pairs / refine_batch /
estimate_homography_batch), both input types, both sub-sampling rules and the shapes where the kernels' indexing changes.
`max_levels` and `max_iters` isolate steps: max_levels=1, max_iters=k is exactly k steps on the finest level;
max_iters=1 is one step on every level.

Metric: the largest distance, in full-resolution pixels, between where the device's and the oracle's transforms put the
frame's four corners (corner_deviation); and |cc_device - cc_oracle| (cc = rho at the start of the last step).

Tolerances, derived rather than tuned.  The device keeps the parameters in double and sums in double, but casts a, b, tx, ty
to float32 and evaluates every sample position in float32.  The cast of a (~1) costs 2^-24 relative, i.e. up to
6e-8 * |x - c| px at a level pixel x; the position arithmetic about as much again: a systematic ~1.2e-7 * half-diagonal px
in the positions the sums see.  A Gauss-Newton step lands where those sums point, so the step inherits that offset: the
floor is ~4e-5 px at 512 x 512 and ~4e-4 px at 24 MP (6000 x 4000), in full-resolution pixels at any sub-sampling (a level
pixel is s * 2^l of them, its half-diagonal that much shorter).  Gray image and pyramid in float32 (relative 1e-7 of
values) and the float32 interpolation add far less.  Targets:
  * one step:  5e-5 px up to 512 x 512 pixels, 1e-3 px above (the 24 MP floor plus the float32 sample-set edge);
  * converged: 2e-3 px, 5e-3 px at 24 MP -- the stop rule (2e-3 px on the level, or rho stalls) may end a level one step
    earlier or later on either side, so the iteration counts may differ by one per level;
  * rho: 1e-5.
A bias of the kind the ground-truth tests (0.2 px) cannot see -- a gradient scaled, taken a sample off, a row too many at
the valid-region edge, a wrong sample step -- moves a step by 1e-3 .. 1e-1 px, far above these.

Set ECC_ORACLE_REPORT=<path> to write the largest deviation seen per test group as JSON."""
import json
import os

import numpy as np
import pytest

from ecc_pairs import invert, make_pair, similarity, texture
from oracle import ecc_oracle as eo

pytestmark = pytest.mark.gpu

TOL_RHO = 1e-5
_WORST = {}


def tol_step(h, w):
    return 5e-5 if h * w <= 512 * 512 else 1e-3


def tol_converged(h, w):
    return 5e-3 if h * w >= 20e6 else 2e-3


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    yield hiplib
    path = os.environ.get("ECC_ORACLE_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump(_WORST, fh, indent=1, sort_keys=True)


def _record(group, dev, drho):
    w = _WORST.setdefault(group, {"corner_px": 0.0, "rho": 0.0})
    w["corner_px"] = max(w["corner_px"], float(dev))
    w["rho"] = max(w["rho"], float(drho))


def check(group, M, cc, it, r, h, w, tol, iters="exact", M_want=None, cc_want=None):
    """Device result (M, cc, it) against the oracle's Result r."""
    M_want = r.M if M_want is None else M_want
    cc_want = r.cc if cc_want is None else cc_want
    dev = eo.corner_deviation(M, M_want, h, w)
    drho = abs(cc - cc_want)
    _record(group, dev, drho)
    assert dev < tol and drho < TOL_RHO, (group, dev, tol, cc, cc_want, it, r)
    if iters == "exact":
        assert it == r.iters, (it, r)
    elif iters == "per_level":
        assert abs(it - r.iters) <= len(r.level_iters), (it, r)


class Frames:
    """Frames in device memory: the reference first, then the moving frames."""

    def __init__(self, L, ref, movs):
        self.nb = ref.nbytes
        self.buf = L.DeviceBuffer((1 + len(movs)) * self.nb)
        self.buf.upload(ref)
        for k, m in enumerate(movs):
            self.buf.upload(m, (k + 1) * self.nb)
        self.ref = self.buf.ptr
        self.movs = [self.buf.ptr + (k + 1) * self.nb for k in range(len(movs))]


def aligner(L, fr, shape, dtype, s=1, area=False, max_levels=0):
    al = L.Aligner(shape[0], shape[1], dtype, subsample=s, max_levels=max_levels, fast=not area)
    al.set_reference(fr.ref)
    return al


def pyr(img, s, area, max_levels=0):
    return eo.frame_pyramid(img, s, area, max_levels)


SUBPIXEL = (0.05, 1.0002, 0.31, -0.17)
C4_STEP = (0.02, 1.0001, 0.37, -0.21)               # one step of the config-4 sequence
KNOWN = [(0.5, 1.003, 7.3, -4.6), (-0.8, 0.994, -12.4, 9.7), C4_STEP, (1.28, 1.0064, 23.7, -13.4)]


def pair(oracle, motion, h, w, dtype=np.uint8, noise=2.0, seed=0):
    T = similarity(*motion, (w - 1) / 2, (h - 1) / 2)
    ref, mov = make_pair(oracle, T, h=h, w=w, noise=noise, seed=seed, dtype=dtype)
    return T, ref, mov


# ------------------------------------------------------------------------------------------------------ single steps
# (h, w, dtype, s, area, motion): u8 and full-range u16, both rules with s in 1..4, odd and ragged sizes, the smallest grid
ONE_LEVEL = [
    (512, 512, np.uint8, 1, False, (0.0, 1.0, 0.0, 0.0)),
    (512, 512, np.uint8, 1, False, SUBPIXEL),
    (512, 512, np.uint16, 1, False, C4_STEP),
    (387, 509, np.uint16, 1, False, SUBPIXEL),
    (130, 1031, np.uint8, 1, False, C4_STEP),
    (512, 512, np.uint8, 2, True, SUBPIXEL),
    (387, 509, np.uint16, 2, False, C4_STEP),
    (387, 509, np.uint8, 3, True, SUBPIXEL),
    (130, 1031, np.uint16, 3, False, SUBPIXEL),
    (512, 512, np.uint16, 4, True, C4_STEP),
    (387, 509, np.uint8, 4, False, SUBPIXEL),
    (32, 48, np.uint8, 2, False, SUBPIXEL),            # 16 x 24 after sub-sampling: the smallest accepted grid
    (48, 64, np.uint16, 3, True, SUBPIXEL),            # 16 x 21
]


@pytest.mark.parametrize("h,w,dtype,s,area,motion", ONE_LEVEL)
def test_exactly_k_steps_on_one_level(L, oracle, h, w, dtype, s, area, motion):
    T, ref, mov = pair(oracle, motion, h, w, dtype)
    fr = Frames(L, ref, [mov])
    al = aligner(L, fr, (h, w), dtype, s, area, max_levels=1)
    lr, lm = pyr(ref, s, area, 1), pyr(mov, s, area, 1)
    try:
        for k in (1, 2, 3):
            ms, ccs, its = al.estimate_batch(fr.movs, max_iters=k)
            r = eo.solve_pyramids(lr, lm, s=s, max_iters=k)
            check("one_level_k_steps", ms[0], ccs[0], its[0], r, h, w, tol_step(h, w))
    finally:
        al.close()


def test_host_entry_single_steps(L, oracle):
    """mi_ecc_similarity (host frames) takes the same steps."""
    T, ref, mov = pair(oracle, KNOWN[0], 512, 512)
    lr, lm = pyr(ref, 1, False), pyr(mov, 1, False)
    for levels, k in ((1, 1), (1, 2), (0, 1)):
        M, cc, it = L.ecc_similarity(ref, mov, max_levels=levels, max_iters=k)
        r = eo.solve_pyramids(lr[:levels] if levels else lr, lm[:levels] if levels else lm, max_iters=k)
        check("one_level_k_steps" if levels else "one_step_per_level", M, cc, it, r, 512, 512, tol_step(512, 512))


# (h, w, dtype, s, area, motion)
PER_LEVEL = [
    (512, 512, np.uint8, 1, False, KNOWN[0]),
    (512, 512, np.uint16, 1, False, KNOWN[1]),
    (512, 512, np.uint8, 2, True, KNOWN[2]),
    (512, 512, np.uint8, 2, False, KNOWN[3]),
    (387, 509, np.uint8, 1, False, KNOWN[3]),
    (387, 509, np.uint16, 2, True, KNOWN[0]),
    (387, 509, np.uint8, 3, False, KNOWN[1]),
    (130, 1031, np.uint16, 1, False, KNOWN[0]),
    (130, 1031, np.uint8, 4, True, KNOWN[2]),
]


@pytest.mark.parametrize("h,w,dtype,s,area,motion", PER_LEVEL)
def test_one_step_on_every_level(L, oracle, h, w, dtype, s, area, motion):
    T, ref, mov = pair(oracle, motion, h, w, dtype)
    fr = Frames(L, ref, [mov])
    al = aligner(L, fr, (h, w), dtype, s, area)
    try:
        ms, ccs, its = al.estimate_batch(fr.movs, max_iters=1)
    finally:
        al.close()
    r = eo.solve_pyramids(pyr(ref, s, area), pyr(mov, s, area), s=s, max_iters=1)
    assert r.level_iters == [1] * len(r.level_iters)
    check("one_step_per_level", ms[0], ccs[0], its[0], r, h, w, tol_step(h, w))


# ------------------------------------------------------------------------------------------------- converged estimates
CONVERGED = [
    (512, 512, np.uint8, 1, False, KNOWN[0], 60),
    (512, 512, np.uint8, 1, False, KNOWN[1], 60),
    (512, 512, np.uint16, 1, False, KNOWN[2], 60),
    (512, 512, np.uint8, 1, False, KNOWN[3], 60),
    (512, 512, np.uint8, 1, False, (15.0, 1.0, 30.0, 20.0), 150),
    (512, 512, np.uint16, 2, True, KNOWN[3], 60),
    (512, 512, np.uint8, 4, False, KNOWN[0], 60),
    (387, 509, np.uint8, 2, False, KNOWN[1], 60),
    (387, 509, np.uint16, 3, True, KNOWN[2], 60),
    (130, 1031, np.uint8, 1, False, KNOWN[0], 60),
    (130, 1031, np.uint16, 2, True, KNOWN[2], 60),
    (32, 48, np.uint16, 2, True, SUBPIXEL, 60),
]


@pytest.mark.parametrize("h,w,dtype,s,area,motion,iters", CONVERGED)
def test_converged_estimate(L, oracle, h, w, dtype, s, area, motion, iters):
    T, ref, mov = pair(oracle, motion, h, w, dtype, noise=5.0)
    fr = Frames(L, ref, [mov])
    al = aligner(L, fr, (h, w), dtype, s, area)
    try:
        ms, ccs, its = al.estimate_batch(fr.movs, max_iters=iters)
    finally:
        al.close()
    r = eo.solve_pyramids(pyr(ref, s, area), pyr(mov, s, area), s=s, max_iters=iters)
    check("converged", ms[0], ccs[0], its[0], r, h, w, tol_converged(h, w), iters="per_level")


# --------------------------------------------------------------------------------------------------------------- 24 MP
@pytest.fixture(scope="module")
def pair24(oracle):
    """One 6000 x 4000 u8 pair (24 MP: sample step 8 on level 0 at s = 1, 4 at s = 2)."""
    T = similarity(0.3, 1.002, 9.0, -6.0, 2999.5, 1999.5)
    return make_pair(oracle, T, h=4000, w=6000, noise=2.0, seed=4)


@pytest.mark.parametrize("s,area", [(1, False), (2, True)])
def test_24mp_pair_step_by_step_and_converged(L, pair24, s, area):
    """24 MP (slow: about half a minute of oracle time each): the sample step is > 1 on the finest levels."""
    ref, mov = pair24
    h, w = ref.shape[:2]
    lr, lm = pyr(ref, s, area), pyr(mov, s, area)
    assert eo.sample_step(lr[0].size) == (8 if s == 1 else 4)
    fr = Frames(L, ref, [mov])
    try:
        for levels in (len(lr), 1):   # one step on every level; one step on level 0 from the identity
            al = aligner(L, fr, (h, w), np.uint8, s, area, max_levels=levels)
            try:
                ms, ccs, its = al.estimate_batch(fr.movs, max_iters=1)
            finally:
                al.close()
            r = eo.solve_pyramids(lr[:levels], lm[:levels], s=s, max_iters=1)
            check("24mp_one_step", ms[0], ccs[0], its[0], r, h, w, tol_step(h, w))
        al = aligner(L, fr, (h, w), np.uint8, s, area)
        try:
            ms, ccs, its = al.estimate_batch(fr.movs)
        finally:
            al.close()
        r = eo.solve_pyramids(lr, lm, s=s)
        check("24mp_converged", ms[0], ccs[0], its[0], r, h, w, tol_converged(h, w), iters="per_level")
    finally:
        fr.buf.free()


# -------------------------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("area", [False, True])
def test_batch_of_five_at_subsample_two_with_a_flat_frame(L, oracle, area):
    """n > 1 at s = 2: the levels 0 and 1 of all frames come from ecc_pyramid2_batch."""
    h, w = 387, 509
    movs = []
    for k, motion in enumerate([KNOWN[0], KNOWN[1], None, SUBPIXEL, KNOWN[3]]):
        if motion is None:
            movs.append(np.full((h, w, 3), 90, np.uint8))
            continue
        T, ref, m = pair(oracle, motion, h, w, seed=6)      # the same seed: the same reference frame
        movs.append(m)
    fr = Frames(L, ref, movs)
    al = aligner(L, fr, (h, w), np.uint8, 2, area)
    lr = pyr(ref, 2, area)
    try:
        for iters, group, tol, rule in ((1, "batch5_one_step_per_level", tol_step(h, w), "exact"),
                                        (60, "batch5_converged", tol_converged(h, w), "per_level")):
            ms, ccs, its = al.estimate_batch(fr.movs, max_iters=iters)
            for k, m in enumerate(movs):
                r = eo.solve_pyramids(lr, pyr(m, 2, area), s=2, max_iters=iters)
                if k == 2:
                    assert r.failed and ccs[k] == -2.0 and np.array_equal(ms[k], [[1, 0, 0], [0, 1, 0]]), (ms[k], ccs[k])
                    continue
                check(group, ms[k], ccs[k], its[k], r, h, w, tol, iters=rule)
    finally:
        al.close()


@pytest.mark.parametrize("s", [1, 2])
def test_batch_of_128_frames_every_frame_its_own_result(L, oracle, s):
    """The largest batch: every frame (blockIdx.y up to 127: its partial sums, ticket and pyramid slot) gets its own
    motion's result; at s = 2 the pyramids come from one ecc_pyramid2_batch launch over 128 frame pointers."""
    h, w = 96 * s, 128 * s
    n = 128
    rng = np.random.default_rng(12)
    base = np.repeat(texture(h, w, 31)[:, :, None], 3, 2)
    ref = np.clip(base + rng.normal(0, 2, base.shape), 0, 255).astype(np.uint8)
    src = np.clip(base, 0, 255).astype(np.uint8)
    movs = []
    for k in range(n):
        th, sc = rng.uniform(-0.6, 0.6), 1 + rng.uniform(-2e-3, 2e-3)
        tx, ty = rng.uniform(-2.5, 2.5, 2) * s
        T = similarity(th, sc, tx, ty, (w - 1) / 2, (h - 1) / 2)
        m = oracle.warp_affine(src, T, border_mode=oracle.BORDER_REPLICATE).astype(np.float64)
        movs.append(np.clip(m + rng.normal(0, 2, m.shape), 0, 255).astype(np.uint8))
    fr = Frames(L, ref, movs)
    al = aligner(L, fr, (h, w), np.uint8, s)
    try:
        ms, ccs, its = al.estimate_batch(fr.movs)
    finally:
        al.close()
    lr = pyr(ref, s, False)
    for k in range(n):
        r = eo.solve_pyramids(lr, pyr(movs[k], s, False), s=s)
        check("batch128_converged", ms[k], ccs[k], its[k], r, h, w, tol_converged(h, w), iters="per_level")


# ---------------------------------------------------------------------------------------------------------------- pairs
def test_pairs_chain_and_a_self_reference(L, oracle):
    """estimate_pairs: frame k against frame k - 1 (the templates are pyramids of the batch, `tslot`), frame 0 against
    itself (the identity, cc = 1)."""
    h, w = 384, 512
    frames = []
    for k in range(6):
        d = k - 2.5
        T, ref, mov = pair(oracle, (0.15 * d, 1 + 4e-4 * d, 1.9 * d, -1.2 * d), h, w, seed=14)
        frames.append(mov)
    ref_of = [0, 0, 1, 2, 3, 4]
    fr = Frames(L, frames[0], frames)
    al = L.Aligner(h, w, np.uint8, subsample=2)
    try:
        ms, ccs, its = al.estimate_pairs(fr.movs, ref_of)
    finally:
        al.close()
    lv = [pyr(f, 2, False) for f in frames]
    for k in range(6):
        r = eo.solve_pyramids(lv[ref_of[k]], lv[k], s=2)
        check("pairs_converged", ms[k], ccs[k], its[k], r, h, w, tol_converged(h, w), iters="per_level")
    assert eo.corner_deviation(ms[0], [[1, 0, 0], [0, 1, 0]], h, w) < 1e-6 and abs(ccs[0] - 1) < 1e-6


# --------------------------------------------------------------------------------------------------------------- refine
@pytest.mark.parametrize("levels", [1, 2])
def test_refine_from_perturbed_starts(L, oracle, levels):
    """refine_batch: M_init -> the starting W on level levels - 1 (translation / (s * 2^level)); starts 2 px and 0.2 deg off;
    a motion that puts a third of the frame outside (the valid region changes as the iteration moves); a start that puts the
    frame entirely off the template fails cleanly, as the oracle says it does."""
    h, w = 512, 512
    c = ((w - 1) / 2, (h - 1) / 2)
    movs, inits = [], []
    for motion, off in [(KNOWN[0], (0.2, 2.0, -2.0)), (KNOWN[1], (-0.2, -2.0, 2.0)), ((0.0, 1.0, 170.0, 0.0), (0.2, 2.0, -2.0)),
                        (SUBPIXEL, None)]:
        T, ref, m = pair(oracle, motion, h, w, seed=8)      # the same seed: the same reference frame
        movs.append(m)
        if off is None:
            inits.append(np.array([[1.0, 0.0, 3 * w], [0.0, 1.0, 0.0]]))
        else:
            th, s_, tx, ty = motion
            inits.append(invert(similarity(th + off[0], s_, tx + off[1], ty + off[2], *c)))
    fr = Frames(L, ref, movs)
    al = aligner(L, fr, (h, w), np.uint8, 2)
    try:
        ms, ccs, its = al.refine_batch(fr.movs, np.array(inits), levels=levels, max_iters=20)
    finally:
        al.close()
    lr = pyr(ref, 2, False)
    for k, m in enumerate(movs):
        r = eo.solve_pyramids(lr, pyr(m, 2, False), s=2, max_iters=20, M_init=inits[k], levels=levels)
        assert len(r.level_iters) == levels
        if k == 3:
            assert r.failed and ccs[k] == -2.0 and np.array_equal(ms[k], [[1, 0, 0], [0, 1, 0]]), (ms[k], ccs[k], r)
            continue
        check("refine_converged", ms[k], ccs[k], its[k], r, h, w, tol_converged(h, w), iters="per_level")


# ----------------------------------------------------------------------------------------------------------- homography
def _projective_pair(oracle, h, w, persp):
    cx, cy = (w - 1) / 2, (h - 1) / 2
    S = np.vstack([similarity(0.4, 1.003, 6.0, -4.0, cx, cy), [0, 0, 1]])
    P = np.array([[1, 0, 0], [0, 1, 0], [persp[0], persp[1], 1]], float)
    C, Ci = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]]), np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
    T = S @ C @ P @ Ci
    T /= T[2, 2]
    base = np.clip(np.repeat(texture(h, w, 17)[:, :, None], 3, 2), 0, 255).astype(np.uint8)
    rng = np.random.default_rng(9)
    mov = oracle.warp_perspective(base, T, border_mode=oracle.BORDER_REPLICATE)
    ref = np.clip(base + rng.normal(0, 2, base.shape), 0, 255).astype(np.uint8)
    mov = np.clip(mov + rng.normal(0, 2, base.shape), 0, 255).astype(np.uint8)
    return ref, mov


@pytest.mark.parametrize("s", [1, 2])
def test_homography_projective_and_pure_similarity(L, oracle, s):
    """estimate_homography_batch: the 8-DoF refinement (ecc_accumulate_h, normalised coordinates) and its read-out, on a
    projective pair (the refinement is kept) and on a pure similarity (kept or not on a near-equal rho: the corner metric
    does not care which)."""
    h, w = 384, 512
    for persp, group in (((4.8e-5, -2.4e-5), "homography_projective"), ((0.0, 0.0), "homography_similarity")):
        ref, mov = _projective_pair(oracle, h, w, persp)
        fr = Frames(L, ref, [mov])
        al = aligner(L, fr, (h, w), np.uint8, s)
        try:
            ms, ccs, its = al.estimate_homography_batch(fr.movs)
        finally:
            al.close()
        r = eo.solve_pyramids(pyr(ref, s, False), pyr(mov, s, False), s=s, homography=True)
        if persp[0]:
            assert r.h_used
        check(group, ms[0], ccs[0], its[0], r, h, w, tol_converged(h, w), iters=None, M_want=r.M9, cc_want=r.cc9)
