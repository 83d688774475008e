"""GPU: the phase-correlation start of the estimator (csrc/kernels_phase.hpp: pc_prepare, pc_fft_lines, pc_cross_power,
pc_peak; pc_fft2 / pc_spectrum / pc_correlate, mi_aligner_set_phase_init and the start-up block of aligner_solve in
capi.hip) stage by stage against its float64 statement (tests/phase_restatement.py), at the shapes where a hand-written
DFT goes wrong.  tests/test_phase_restatement.py proves on the CPU that every case used here is decided.

STAGES (mi_phase_correlate_tap_device).  Every stage is held twice: to the float64 statement of THAT STAGE applied to the
kernel's own previous stage (tapped), so that one wrong stage shows by itself, and end to end to the whole float64
statement.  Spectra relative to the largest bin, the surface relative to P Q, the cross-power absolute (|R| = 1).

BOUNDS.  None is taken from a kernel.  For each case and quantity the float32 statement (the kernels' operations in the
kernels' order, twiddles and window correctly rounded) is measured against the float64 statement on the CPU
(phase_cases.deviations); the kernel's bound is FACTOR = 8 times that, and where that deviation is exactly 0 the
comparison is ==.  Why 8: the device's sincospif / cospif are good to an ulp or two rather than correctly rounded, and a
maximum over up to a million rounding-noise terms moves by tens of per cent between two equally correct programs; a wrong
index, stride or twiddle is six orders above.  (dx, dy, response) share one bound per case, 8 x the largest of their three
deviations: they are quotients of the same 25 surface values.

Deviation of the float32 statement from the float64 one (the bound is 8 x), measured on the CPU:

  case        windowed  spectrum  spectrum  cross-p.  cross-p.  surface   surface   dx, dy,
                        own       whole     own       whole     own       whole     response
  3x3         0         0         0         0         0         0         0         0
  5x7         3.7e-08   7.1e-08   6.6e-08   9.9e-08   1.8e-06   3.5e-08   1.0e-07   1.1e-07
  3x1000      5.5e-08   3.4e-08   3.5e-08   1.2e-07   6.4e-06   7.2e-08   6.3e-08   6.6e-08
  1000x3      5.2e-08   5.2e-08   5.3e-08   1.2e-07   4.4e-06   1.0e-07   1.2e-07   1.4e-07
  513x9       8.2e-08   7.5e-08   7.1e-08   1.5e-07   2.6e-05   3.2e-08   2.8e-08   6.8e-08
  9x513       8.2e-08   9.8e-08   8.3e-08   1.4e-07   9.3e-06   1.8e-08   2.7e-08   1.8e-07
  64x64       7.1e-08   4.1e-08   4.1e-08   1.4e-07   8.4e-06   8.0e-08   7.0e-08   1.4e-07
  65x64       8.1e-08   5.7e-08   5.8e-08   1.5e-07   1.4e-05   7.6e-08   7.9e-08   2.2e-07
  250x375     9.4e-08   6.0e-08   6.1e-08   1.6e-07   4.6e-05   9.0e-08   8.9e-08   1.0e-07
  1023x600    1.0e-07   5.3e-08   5.4e-08   1.7e-07   3.0e-04   8.7e-08   8.5e-08   7.2e-08
  1024x1024   1.0e-07   4.1e-08   4.3e-08   1.6e-07   1.6e-04   9.8e-08   9.9e-08   1.0e-07
  (spectrum: the larger of ref and mov.  "cross-p. whole" is large because a small bin divides the spectra's noise by its
  magnitude; the smallest bin of these cases is 2.3e-10 of the largest.)
  results through phase_correlate: zero shift 9.7e-08 .. 2.1e-07, +-1 / +-2 px 1.8e-08 .. 2.1e-07, +-(P / 2 - 3) and
  +-(Q / 2 - 3) 9.3e-08 .. 1.5e-06 (a response of 0.1: half the planes overlap), the fractional shift of a smoothed field
  4.0e-06, unrelated 1000 x 1000 planes 2.1e-06 (the centroid; the response alone 1.2e-09).

EXACT, no bound: pc_peak against the statement's peak search on the tapped surface (both float64, one order of
operations); 3 x 3 (Hann leaves the centre pixel: the surface is exactly P Q at the origin, the result (0, 0, 1)); 2 x 2 and
2 x 9 (a window of zeros: every tap 0, the result (0, 0, 0)); a plane against itself: the cross-power's imaginary part
x.y y.x - x.x y.y is exactly 0 in every bin -- with contraction on it is the rounding error of a product -- and its real
part re * (1 / |re|) is 1 or 1 - 2^-24.  (Not exactly 1: x * (1 / x) != 1 for one float32 in seven, so the surface of a
plane against itself is P Q only to 2^-24 and its result is held to the statement within the bound like every other.)

THE ALIGNER: which level the correlation runs on, the 0.02 response gate, the batch's per-frame planes and outputs, the
cached reference spectrum, the switch, the paths that ignore it and the Python layer, with the tolerances of
tests/test_gpu_ecc.py (0.005 deg, 0.2 px, 1e-4) against the truth and == between runs (the reductions are deterministic)."""
import numpy as np
import pytest

import phase_cases as pc
import phase_restatement as pr
from ecc_pairs import decompose, invert, make_pair, similarity

pytestmark = pytest.mark.gpu

STAGES = list(pc.STAGE_CASES)
_taps = {}


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


def taps(L, name):
    """every tap of one case, once: windowed_ref is the windowed-mov tap of the swapped pair"""
    if name not in _taps:
        ref, mov = pc.planes(name)
        t = {k: L.phase_tap(ref, mov, getattr(L, "PC_TAP_" + k.upper()))
             for k in ("windowed_mov", "spectrum_ref", "spectrum_mov", "cross_power", "surface")}
        t["windowed_ref"] = L.phase_tap(mov, ref, L.PC_TAP_WINDOWED_MOV)
        t["result"] = L.phase_correlate(ref, mov)
        _taps[name] = t
    return _taps[name]


def check(failed, label, got, want, dev, scale=1.0):
    ok, err = pc.held(got, want, dev, scale)
    print(f"{label}: measured {err:.3e}, statement's own deviation {dev:.3e}, bound {pc.FACTOR * dev:.3e}{'' if ok else '  <-- MISSED'}")
    if not ok:
        failed.append(label)


def check_result(failed, name, got, label="result"):
    d, s64 = pc.deviations(name), pc.statement(name, np.float64)
    for k, g, dev in zip(("dx", "dy", "response"), got, (d.dx, d.dy, d.response)):
        check(failed, f"{name} {label} {k}", g, getattr(s64, k), d.result if dev != 0.0 else 0.0)


# ------------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("name", STAGES)
def test_windowed_plane(L, name):
    s64, d, failed = pc.statement(name, np.float64), pc.deviations(name), []
    t = taps(L, name)
    assert t["windowed_mov"].shape == (s64.P, s64.Q) and t["windowed_mov"].dtype == np.complex64
    scale = float(np.abs(s64.windowed_mov).max())
    check(failed, f"{name} windowed mov", t["windowed_mov"], s64.windowed_mov, d.windowed, scale)
    check(failed, f"{name} windowed ref", t["windowed_ref"], s64.windowed_ref, d.windowed_ref, float(np.abs(s64.windowed_ref).max()))
    h, w = pc.planes(name)[0].shape
    pad = t["windowed_mov"].copy()
    pad[:h, :w] = 0
    assert not pad.any() and not t["windowed_mov"].imag.any()        # the padding and the imaginary part are exactly 0
    assert not failed, failed


@pytest.mark.parametrize("name", STAGES)
def test_forward_spectra(L, name):
    s64, d, failed = pc.statement(name, np.float64), pc.deviations(name), []
    t = taps(L, name)
    for k in ("ref", "mov"):
        own = pc.own_stage("spectrum", t["windowed_" + k])
        check(failed, f"{name} spectrum {k} own", t["spectrum_" + k], own, getattr(d, "own_spectrum_" + k), float(np.abs(own).max()))
        whole = getattr(s64, "spectrum_" + k)
        check(failed, f"{name} spectrum {k} whole", t["spectrum_" + k], whole, getattr(d, "e2e_spectrum_" + k), float(np.abs(whole).max()))
    assert not failed, failed


@pytest.mark.parametrize("name", STAGES)
def test_cross_power(L, name):
    s64, d, failed = pc.statement(name, np.float64), pc.deviations(name), []
    t = taps(L, name)
    check(failed, f"{name} cross-power own", t["cross_power"], pc.own_stage("cross_power", t["spectrum_mov"], t["spectrum_ref"]),
          d.own_cross_power)
    check(failed, f"{name} cross-power whole", t["cross_power"], s64.cross_power, d.e2e_cross_power)
    assert not failed, failed


@pytest.mark.parametrize("name", STAGES)
def test_surface(L, name):
    s64, d, failed = pc.statement(name, np.float64), pc.deviations(name), []
    t = taps(L, name)
    PQ = float(s64.P * s64.Q)
    check(failed, f"{name} surface own", t["surface"], pc.own_stage("surface", t["cross_power"]), d.own_surface, PQ)
    check(failed, f"{name} surface whole", t["surface"], s64.surface, d.e2e_surface, PQ)
    check(failed, f"{name} surface imaginary part", t["surface"].imag, 0.0, d.own_surface, PQ)
    assert not failed, failed


@pytest.mark.parametrize("name", STAGES)
def test_peak_and_result(L, name):
    """pc_peak == the statement's peak search on the tapped surface (float64 both, the same order of operations); the
    result against the whole float64 statement"""
    t, failed = taps(L, name), []
    dx, dy, response, at = pr.peak(t["surface"].real)
    print(name, "result", t["result"], "statement on the tapped surface", (dx, dy, response), "peak", at)
    assert t["result"] == (dx, dy, response) and at == pc.statement(name, np.float64).peak
    check_result(failed, name, t["result"])
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("name", STAGES)
def test_a_plane_against_itself(L, name):
    """phase_correlate(a, a): identical spectra, a cross-power with an imaginary part of exactly 0 (the build flag) and a
    real part of 1 or 1 - 2^-24, the surface within its bounds, the result (0, 0, 1) within what they allow.  Measured on
    the MI355X: |response - 1| from 7e-12 (1024 x 1024) to 2.8e-8 (5 x 7), |dx|, |dy| under 1e-30."""
    same, failed = pc.SAME + name, []
    t, d, s64 = taps(L, same), pc.deviations(pc.SAME + name), pc.statement(pc.SAME + name, np.float64)
    R = t["cross_power"]
    one_less = np.float32(1.0) - np.float32(2.0 ** -24)
    print(same, "bins with im != 0:", np.count_nonzero(R.imag), "bins at 1 - 2^-24:", np.count_nonzero(R.real == one_less), "of", R.size)
    assert np.array_equal(t["spectrum_ref"], t["spectrum_mov"])
    assert not R.imag.any() and np.isin(R.real, [np.float32(1.0), one_less]).all()
    PQ = float(s64.P * s64.Q)
    check(failed, f"{same} surface own", t["surface"], pc.own_stage("surface", R), d.own_surface, PQ)
    check(failed, f"{same} surface whole", t["surface"], s64.surface, d.e2e_surface, PQ)
    # the result against (0, 0, 1) from the surface's bound b (relative to P Q), not from a measured deviation -- the
    # float32 statement's own is the sum of 24 values of either sign near 1e-9 and happens to be 6e-12 at 250 x 375:
    # response = (sum of 25 values) / (P Q) moves by <= 25 b; the centroid is sum(v * offset) / sum(v) with |offset| <= 2
    # and 0 at the origin, so it moves by <= 48 b / (1 - 25 b).  b = 0 (3 x 3) is ==.
    b = pc.FACTOR * d.e2e_surface
    dx, dy, response = t["result"]
    print(same, "result", t["result"], "bounds", 48 * b / (1 - 25 * b), 25 * b)
    assert pr.peak(t["surface"].real)[:3] == t["result"]
    assert abs(dx) <= 48 * b / (1 - 25 * b) and abs(dy) <= 48 * b / (1 - 25 * b) and abs(response - 1.0) <= 25 * b
    assert not failed, failed


def test_three_by_three_is_exact(L):
    t = taps(L, "3x3")
    want = np.zeros((4, 4), np.complex64)
    want[0, 0] = 16.0
    assert np.array_equal(t["surface"], want) and np.array_equal(t["cross_power"], np.ones((4, 4), np.complex64))
    assert t["result"] == (0.0, 0.0, 1.0)


@pytest.mark.parametrize("shape", [(2, 2), (2, 9)])
def test_a_window_of_zeros_gives_zero_everywhere(L, shape):
    a = pc.noise_pair(*shape, (0, 0))[0]
    for what in range(5):
        plane = L.phase_tap(a, a, what)
        assert plane.shape == (2, pr.pow2(shape[1])) and not plane.any(), what
    assert L.phase_correlate(a, a) == (0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------ results
@pytest.mark.parametrize("name", list(pc.RESULT_CASES))
def test_result_of_the_public_entry(L, name):
    failed = []
    got = L.phase_correlate(*pc.planes(name))
    s64 = pc.statement(name, np.float64)
    print(name, "got", got, "statement", (s64.dx, s64.dy, s64.response))
    check_result(failed, name, got)
    assert not failed, failed


def test_unrelated_planes_have_the_statements_response(L):
    """(under 0.01 in float64, tests/test_phase_restatement.py: the aligner's 0.02 gate is decided)"""
    failed = []
    got = L.phase_correlate(*pc.planes(pc.UNRELATED))
    d, s64 = pc.deviations(pc.UNRELATED), pc.statement(pc.UNRELATED, np.float64)
    print("unrelated", got, (s64.dx, s64.dy, s64.response))
    check(failed, "unrelated response", got[2], s64.response, d.result)
    assert not failed and got[2] < 0.01, failed


def test_argument_checks_of_both_entries(L):
    lib = L.load()
    buf = L.DeviceBuffer(2 * 4 * 1025 * 2)
    out3 = (L.C.c_double * 3)()
    host = np.empty((2048, 2), np.complex64)
    p, q = buf.ptr, buf.ptr + 4 * 1025 * 2
    try:
        for args, rc, msg in [((p, q, 1, 8), L.MI_ERR_INVALID, "plane too small"), ((p, q, 8, 1), L.MI_ERR_INVALID, "plane too small"),
                              ((p, q, 1025, 2), L.MI_ERR_UNSUPPORTED, "at most 1024 pixels per side"),
                              ((p, q, 2, 1025), L.MI_ERR_UNSUPPORTED, "at most 1024 pixels per side"),
                              ((None, q, 8, 8), L.MI_ERR_INVALID, "null argument"), ((p, None, 8, 8), L.MI_ERR_INVALID, "null argument")]:
            assert lib.mi_phase_correlate_device(0, None, *args, out3) == rc and msg in L.last_error(), args
            assert lib.mi_phase_correlate_tap_device(0, None, *args, L.PC_TAP_SURFACE, host.ctypes.data) == rc and msg in L.last_error(), args
        assert lib.mi_phase_correlate_device(0, None, p, q, 8, 8, None) == L.MI_ERR_INVALID and "null argument" in L.last_error()
        assert lib.mi_phase_correlate_tap_device(0, None, p, q, 8, 8, L.PC_TAP_SURFACE, None) == L.MI_ERR_INVALID
        assert "null argument" in L.last_error()
        for what in (-1, 5):
            assert lib.mi_phase_correlate_tap_device(0, None, p, q, 8, 8, what, host.ctypes.data) == L.MI_ERR_INVALID
            assert "unknown phase-correlation tap" in L.last_error()
    finally:
        buf.free()


# -------------------------------------------------------------------------------------------------------- the aligner
class Frames:
    """frames in one device buffer; .ptr[k]"""

    def __init__(self, L, frames):
        self.nbytes = frames[0].nbytes
        self.buf = L.DeviceBuffer(len(frames) * self.nbytes)
        for k, f in enumerate(frames):
            self.buf.upload(np.ascontiguousarray(f), k * self.nbytes)
        self.ptr = [self.buf.ptr + k * self.nbytes for k in range(len(frames))]

    def free(self):
        self.buf.free()


def outcome(L, fn):
    """what one estimate gave, comparable with ==: the transform's bytes, cc and iterations, or the failure's message"""
    try:
        m, cc, it = fn()
        return (np.asarray(m).tobytes(), float(cc), int(it))
    except L.DeviceError as e:
        return ("failed", str(e))


def errors(m, T, h, w):
    """(angle [deg], scale, mapping of the centre [px]) of the estimate m against the truth: moving = warp(ref, T)"""
    want = invert(T)
    ctr = np.array([(w - 1) / 2, (h - 1) / 2, 1.0])
    return (abs(decompose(m)[0] - decompose(want)[0]), abs(decompose(m)[1] - decompose(want)[1]), np.abs(m @ ctr - want @ ctr).max())


def recovered(m, T, h, w):
    e = errors(m, T, h, w)
    return e[0] < 0.005 and e[1] < 1e-4 and e[2] < 0.2


def fifth(h, w, sign=1, theta=0.3, s=1.002):
    """a translation of a fifth of the long side (and a little of the other)"""
    c = ((w - 1) / 2, (h - 1) / 2)
    return similarity(theta, s, sign * 0.2 * w, -0.02 * h, *c) if w >= h else similarity(theta, s, 0.02 * w, sign * 0.2 * h, *c)


@pytest.mark.parametrize("h,w,dtype,subsample,theta,s", [
    (200, 300, np.uint8, 1, 0.3, 1.002),      # pc_level 0: P x Q = 256 x 512
    (60, 1000, np.uint8, 1, 0.1, 1.001),      # one level (60 / 2 < 48) longer than 512: the coarsest level it is, Q = 1024
    (400, 600, np.uint8, 2, 0.3, 1.002),      # the sub-sampled frame is the 200 x 300 one; the translation is in full pixels
    (200, 300, np.uint16, 1, 0.3, 1.002),
])
def test_level_choice_extends_the_capture_range(L, oracle, h, w, dtype, subsample, theta, s):
    """(768 x 1024, pc_level 1: test_phase_correlation_extends_the_capture_range_of_the_ecc_estimator in test_gpu_ecc.py)"""
    T = fifth(h, w, 1, theta, s)
    fr = Frames(L, make_pair(oracle, T, h=h, w=w, seed=21, noise=2.0, dtype=dtype))
    out = {}
    for phase in (False, True):
        al = L.Aligner(h, w, dtype, subsample=subsample, phase_init=phase)
        al.set_reference(fr.ptr[0])
        try:
            m, cc, _ = al.estimate(fr.ptr[1])
            out[phase] = (*errors(m, T, h, w), cc)
        except L.DeviceError:
            out[phase] = None
        al.close()
    fr.free()
    print((h, w, dtype.__name__, subsample), out)
    good = out[True]
    assert good is not None and good[0] < 0.005 and good[1] < 1e-4 and good[2] < 0.2 and good[3] > 0.9, out
    assert out[False] is None or out[False][2] > 5.0 or out[False][3] < 0.5, out    # the plain estimator does not get there


def test_a_frame_without_a_level_is_unsupported_and_the_handle_stays_plain(L, oracle):
    h, w = 60, 2100                                # one level, 2100 > PC_MAX_N
    c = ((w - 1) / 2, (h - 1) / 2)
    fr = Frames(L, make_pair(oracle, similarity(0.05, 1.0005, 3.0, -2.0, *c), h=h, w=w, seed=21, noise=2.0))
    plain, al = L.Aligner(h, w, np.uint8), L.Aligner(h, w, np.uint8)
    try:
        assert L.load().mi_aligner_set_phase_init(al._h, 1) == L.MI_ERR_UNSUPPORTED
        assert "phase correlation: no pyramid level between 2 and 1024 pixels per side" in L.last_error()
        with pytest.raises(L.InvalidOptionError):
            L.Aligner(h, w, np.uint8, phase_init=True)
        plain.set_reference(fr.ptr[0])
        al.set_reference(fr.ptr[0])
        want = outcome(L, lambda: plain.estimate(fr.ptr[1]))
        assert want[0] != "failed" and outcome(L, lambda: al.estimate(fr.ptr[1])) == want
    finally:
        plain.close()
        al.close()
        fr.free()


def test_a_batch_gives_every_frame_its_own_start(L, oracle):
    """+0.2 w, -0.2 w, +0.2 h, about 0, and an unrelated frame (float64 response 0.0004: under the 0.02 gate, its row is the
    plain estimator's): a frame that got another frame's start, plane or output row cannot pass"""
    h, w = 200, 300
    c = ((w - 1) / 2, (h - 1) / 2)
    Ts = [similarity(0.3, 1.002, 0.2 * w, -5.0, *c), similarity(-0.2, 0.999, -0.2 * w, 4.0, *c),
          similarity(0.1, 1.001, 6.0, 0.2 * h, *c), similarity(0.3, 1.002, 1.5, -2.5, *c)]
    pairs = [make_pair(oracle, T, h=h, w=w, seed=21, noise=2.0) for T in Ts]
    other = make_pair(oracle, similarity(0.0, 1.0, 0.0, 0.0, *c), h=h, w=w, seed=5, noise=2.0)[0]
    fr = Frames(L, [pairs[0][0]] + [p[1] for p in pairs] + [other])
    rows = {}
    for phase in (False, True):
        al = L.Aligner(h, w, np.uint8, phase_init=phase)
        al.set_reference(fr.ptr[0])
        rows[phase] = al.estimate_batch(fr.ptr[1:])
        if phase:
            singles = [outcome(L, lambda k=k: al.estimate(fr.ptr[1 + k])) for k in range(4)]
        al.close()
    fr.free()
    ms, ccs, its = rows[True]
    for k, T in enumerate(Ts):
        print(k, errors(ms[k], T, h, w), ccs[k], its[k], "plain:", errors(rows[False][0][k], T, h, w), rows[False][1][k])
        assert recovered(ms[k], T, h, w) and ccs[k] > 0.9, (k, errors(ms[k], T, h, w), ccs[k])
        assert singles[k] == (ms[k].tobytes(), float(ccs[k]), int(its[k])), k      # and what a single estimate gives
    assert not any(recovered(rows[False][0][k], Ts[k], h, w) for k in range(2))   # the plain estimator does not reach +-0.2 w
    print("unrelated:", ms[4], ccs[4], its[4], "plain:", rows[False][0][4], rows[False][1][4], rows[False][2][4])
    assert np.array_equal(ms[4], rows[False][0][4]) and ccs[4] == rows[False][1][4] and its[4] == rows[False][2][4]


def test_a_new_reference_replaces_the_cached_spectrum(L, oracle):
    """set_reference(A), estimate(B), set_reference(C), estimate(B) == a fresh aligner with reference C"""
    h, w = 200, 300
    c = ((w - 1) / 2, (h - 1) / 2)
    A, B = make_pair(oracle, similarity(0.3, 1.002, 0.2 * w, -5.0, *c), h=h, w=w, seed=21, noise=2.0)
    # (without noise: make_pair would give C the very noise field B has, and the whitened spectra would lock onto it)
    C = make_pair(oracle, similarity(0.3, 1.002, -0.08 * w, 8.0, *c), h=h, w=w, seed=21, noise=0.0)[1]
    fr = Frames(L, [A, B, C])
    al, fresh = L.Aligner(h, w, np.uint8, phase_init=True), L.Aligner(h, w, np.uint8, phase_init=True)
    try:
        al.set_reference(fr.ptr[0])
        first = outcome(L, lambda: al.estimate(fr.ptr[1]))
        al.set_reference(fr.ptr[2])
        second = outcome(L, lambda: al.estimate(fr.ptr[1]))
        fresh.set_reference(fr.ptr[2])
        want = outcome(L, lambda: fresh.estimate(fr.ptr[1]))
    finally:
        al.close()
        fresh.close()
        fr.free()
    assert first[0] != "failed" and want[0] != "failed" and first != want     # B lies 0.2 w from A and 0.28 w from C
    assert second == want


def test_the_switch_turns_the_start_off_and_on_again(L, oracle):
    h, w = 200, 300
    T = fifth(h, w)
    fr = Frames(L, make_pair(oracle, T, h=h, w=w, seed=21, noise=2.0))
    plain, phase, al = L.Aligner(h, w, np.uint8), L.Aligner(h, w, np.uint8, phase_init=True), L.Aligner(h, w, np.uint8, phase_init=True)
    try:
        for a in (plain, phase, al):
            a.set_reference(fr.ptr[0])
        want_plain, want_phase = outcome(L, lambda: plain.estimate(fr.ptr[1])), outcome(L, lambda: phase.estimate(fr.ptr[1]))
        assert want_phase[0] != "failed" and want_plain != want_phase
        assert outcome(L, lambda: al.estimate(fr.ptr[1])) == want_phase
        assert L.load().mi_aligner_set_phase_init(al._h, 0) == L.MI_OK
        assert outcome(L, lambda: al.estimate(fr.ptr[1])) == want_plain
        assert L.load().mi_aligner_set_phase_init(al._h, 1) == L.MI_OK
        assert outcome(L, lambda: al.estimate(fr.ptr[1])) == want_phase
    finally:
        for a in (plain, phase, al):
            a.close()
        fr.free()


def test_refine_and_pairs_ignore_the_start(L, oracle):
    """refine_batch starts from the caller's transforms, estimate_pairs registers against frames of the batch: == with and
    without the option"""
    h, w = 200, 300
    c = ((w - 1) / 2, (h - 1) / 2)
    Ts = [similarity(0.3, 1.002, 0.2 * w, -5.0, *c), similarity(-0.2, 0.999, 7.0, 4.0, *c)]
    pairs = [make_pair(oracle, T, h=h, w=w, seed=21, noise=2.0) for T in Ts]
    fr = Frames(L, [pairs[0][0]] + [p[1] for p in pairs])
    inits = np.array([invert(similarity(0.4, 1.002, 0.2 * w + 1.5, -6.0, *c)), invert(similarity(-0.1, 0.999, 6.0, 5.0, *c))])
    got = {}
    for phase in (False, True):
        al = L.Aligner(h, w, np.uint8, phase_init=phase)
        al.set_reference(fr.ptr[0])
        got[phase] = (al.refine_batch(fr.ptr[1:], inits, levels=2), al.estimate_pairs(fr.ptr, [0, 0, 0]))
        al.close()
    fr.free()
    for a, b in zip(got[False], got[True]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert (got[True][0][1] > 0.9).all()                                      # and the refinement did run


def test_the_python_estimator_passes_the_option_on(L, oracle):
    """align.ecc_estimator(phase_init=True) on host arrays: (moving, reference) -> 1000 matches and moving -> reference"""
    from shinestacker_amd.align import ecc_estimator
    h, w = 200, 300
    T = fifth(h, w)
    ref, mov = make_pair(oracle, T, h=h, w=w, seed=21, noise=2.0)
    n, m = ecc_estimator(phase_init=True)(mov, ref, None, None, {})
    assert n == 1000 and recovered(m, T, h, w), (n, m)
