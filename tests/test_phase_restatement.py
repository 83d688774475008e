"""The NumPy statement of phase correlation (tests/phase_restatement.py) against what is known without it -- np.fft,
the recipe of tests/test_gpu_ecc.py, two analytic cases -- and the conditions under which the cases of
tests/test_gpu_phase_edges.py (tests/phase_cases.py) are DECIDED, proven from the statement alone before a kernel is
asked: a case whose arg-max, wrap sign or cross-power hangs on rounding noise is refused here."""
import numpy as np
import pytest

import phase_cases as pc
import phase_restatement as pr

ALL_CASES = list(pc.STAGE_CASES) + list(pc.RESULT_CASES) + [pc.UNRELATED]


@pytest.mark.parametrize("name", list(pc.STAGE_CASES))
def test_float64_radix2_equals_numpy_fft(name):
    """forward on the windowed plane, inverse (un-normalised) on the cross-power: 1e-13 of the largest bin (rounding alone
    gives 1e-16)"""
    s = pc.statement(name, np.float64)
    want = np.fft.fft2(s.windowed_mov)
    assert pc.rel(s.spectrum_mov, want, np.abs(want).max()) < 1e-13
    want = np.fft.ifft2(s.cross_power) * (s.P * s.Q)
    assert pc.rel(s.surface, want, np.abs(want).max()) < 1e-13


@pytest.mark.parametrize("shape,shift", [((250, 375), (17.0, -9.0)), ((256, 512), (-40.0, 31.0)), ((125, 188), (3.4, 7.7)),
                                         ((300, 300), (0.0, 0.0))])
def test_float64_statement_equals_the_recipe_of_the_ecc_tests(shape, shift):
    """the four cases of test_phase_correlation_equals_its_float64_statement_and_finds_the_shift, its planes, its recipe"""
    from scipy import ndimage
    from test_gpu_ecc import _phase_correlate_numpy, texture
    h, w = shape
    big = ndimage.gaussian_filter(texture(h + 200, w + 200, seed=7).astype(np.float64), 1.0)
    dx, dy = shift
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ref = ndimage.map_coordinates(big, [yy + 100, xx + 100], order=3).astype(np.float32)
    mov = ndimage.map_coordinates(big, [yy + 100 - dy, xx + 100 - dx], order=3).astype(np.float32)
    s = pr.phase_correlate(ref, mov, np.float64)
    want = _phase_correlate_numpy(ref.astype(np.float64), mov.astype(np.float64))
    # two float64 programs of one recipe; the centroid is a quotient of sums of 25 surface values good to 1e-15 P Q
    assert np.abs(np.array([s.dx, s.dy, s.response]) - np.array(want)).max() < 1e-9, ((s.dx, s.dy, s.response), want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("P,Q,y,x", [(4, 4, 1, 1), (8, 16, 3, 5), (2, 1024, 1, 700), (1024, 4, 513, 2)])
def test_an_impulse_has_a_spectrum_of_unit_magnitude_and_its_phase_ramp(dtype, P, Q, y, x):
    """the transform alone, without the window: delta(y, x) -> e^{-2 pi i (u y / P + v x / Q)}"""
    re = np.zeros((P, Q))
    re[y, x] = 1.0
    fr, fi = pr.fft2(re, np.zeros((P, Q)), False, dtype)
    u, v = np.mgrid[0:P, 0:Q]
    want = np.exp(-2j * np.pi * ((u * y % P) / P + (v * x % Q) / Q))
    tol = 1e-14 if dtype == np.float64 else 2e-7   # the twiddles' rounding through log2(P Q) <= 12 products
    assert np.abs(fr + 1j * fi - want).max() < tol
    br, bi = pr.fft2(fr, fi, True, dtype)
    assert np.abs(br + 1j * bi - re * (P * Q)).max() < tol * P * Q


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_three_by_three_leaves_the_centre_pixel_and_a_delta_surface(dtype):
    """Hann of 3 points is (0, 1, 0): one pixel each, R = 1 in every bin, the surface is exactly P Q at the origin and 0
    elsewhere, the result (0, 0, 1)"""
    s = pc.statement("3x3", dtype)
    want = np.zeros((4, 4), complex)
    want[0, 0] = 16.0
    assert np.array_equal(s.surface, want) and (s.dx, s.dy, s.response) == (0.0, 0.0, 1.0)
    assert np.count_nonzero(s.windowed_mov) == 1 and s.windowed_mov[1, 1] == pc.planes("3x3")[1][1, 1]


@pytest.mark.parametrize("shape", [(2, 2), (2, 9)])
def test_a_window_of_all_zeros_gives_zero_everywhere(shape):
    """Hann of 2 points is (0, 0): every stage 0, the first maximum at index 0, the m == 0 branch of the centroid"""
    a = pc.noise_pair(*shape, (0, 0))[0]
    for dtype in (np.float32, np.float64):
        s = pr.phase_correlate(a, a, dtype)
        assert not s.windowed_mov.any() and not s.spectrum_mov.any() and not s.cross_power.any() and not s.surface.any()
        assert (s.dx, s.dy, s.response) == (0.0, 0.0, 0.0) and s.peak == (0, 0)


@pytest.mark.parametrize("name", list(pc.STAGE_CASES))
def test_a_plane_against_itself_has_a_real_cross_power_of_one_or_one_ulp_less(name):
    """What IS exact for phase_correlate(a, a) in float32 with every operation rounded on its own: im = x.y y.x - x.x y.y
    is 0 in every bin (the two products are the same number), re * (1 / sqrt(re re)) is 1 or 1 - 2^-24 (x (1 / x) is not 1
    for every float32 x).  So the surface is P Q at the origin only up to 2^-24, not exactly; dx and dy are 0 to rounding."""
    s = pc.statement(pc.SAME + name, np.float32)
    R = s.cross_power
    assert not R.imag.any() and np.isin(R.real, [np.float32(1.0), np.float32(1.0) - np.float32(2.0 ** -24)]).all()
    assert s.peak == (0, 0) and abs(s.dx) < 1e-12 and abs(s.dy) < 1e-12 and abs(s.response - 1.0) < 2.0 ** -24


@pytest.mark.parametrize("name", ALL_CASES)
def test_the_case_is_decided_before_any_kernel_runs(name):
    s64, s32, d = pc.statement(name, np.float64), pc.statement(name, np.float32), pc.deviations(name)
    P, Q = s64.P, s64.Q
    # 1. where the stages are compared, no cross-power bin is small: none has to be left out of a comparison.  (The result
    #    cases are compared in (dx, dy, response) alone; the smoothed field of the fractional one has bins down to 1e-15.)
    if name in pc.STAGE_CASES:
        assert s64.cross_mag.min() > 1e-12 * s64.cross_mag.max()
    # 2. the arg-max is decided: the maximum exceeds every other value (its own window's included) by > 100 x the bound
    surf = s64.surface.real.copy()
    top = surf[s64.peak]
    surf[s64.peak] = -np.inf
    assert top - surf.max() > 100 * pc.FACTOR * d.e2e_surface * P * Q
    # 3. the sign of the wrap is decided: the centroid is >= 2 px from half the size (its position, before the wrap)
    assert Q / 2 - abs(s64.dx) >= 2.0 and P / 2 - abs(s64.dy) >= 2.0
    # 4. both statements pick the same peak
    assert s32.peak == s64.peak


def test_the_cases_cover_both_signs_and_both_wraps():
    shifts = [v[2] for v in pc.STAGE_CASES.values()]
    assert any(s[0] > 0 for s in shifts) and any(s[0] < 0 for s in shifts)
    assert any(s[1] > 0 for s in shifts) and any(s[1] < 0 for s in shifts)
    for name in pc.RESULT_CASES:
        if name.startswith("half"):
            s = pc.statement(name, np.float64)
            dx, dy = pc.RESULT_CASES[name][1][2]
            assert abs(s.dx - dx) < 1.0 and abs(s.dy - dy) < 1.0 and s.response > 0.05, (name, s.dx, s.dy, s.response)


def test_unrelated_planes_stay_under_the_aligners_gate():
    """the aligner ignores a peak whose response is not above 0.02: 0.01 leaves the gate decided"""
    s = pc.statement(pc.UNRELATED, np.float64)
    assert abs(s.response) < 0.01 and pc.deviations(pc.UNRELATED).response < 1e-3
