"""CPU: the float64 statement of the ECC estimator (oracle/ecc_oracle.py) is itself right -- its Jacobians are the
derivatives of its own warp and sampling, its pyramid is the documented blur, its tables are the documented rules, and it
is a working ECC on its own (recovers known transforms ten times inside the reference's tolerances, fails where the
algorithm says it fails).  Without these, tests/test_gpu_ecc_oracle.py would only show that two implementations agree."""
import numpy as np
import pytest

from ecc_pairs import invert, make_pair, similarity, texture
from oracle import ecc_oracle as eo


# ------------------------------------------------------------------------------------------------------------ Jacobians
def _ramp(h, w, alpha, beta, gamma=100.0):
    """A linear image: its bilinear samples and central differences are exact, so finite differences of
    sample(warp(p)) are the true derivatives the analytic Jacobian claims."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return gamma + alpha * xx + beta * yy


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_similarity_jacobian_equals_finite_differences(seed):
    rng = np.random.default_rng(seed)
    h, w = 301, 417
    img = _ramp(h, w, *rng.uniform(-3, 3, 2))
    cx, cy = eo.centre(h, w)
    th = rng.uniform(-0.05, 0.05)
    p = np.array([np.cos(th) * rng.uniform(0.98, 1.02), np.sin(th), *rng.uniform(-8, 8, 2)])
    x, y = rng.uniform(40, w - 40, 200), rng.uniform(40, h - 40, 200)
    valid, _, gx, gy = eo.sample(img, *eo.warp_sim(p, x, y, cx, cy))
    assert valid.all()
    J = eo.jac_sim(gx, gy, x, y, cx, cy)
    for q in range(4):
        e = np.zeros(4)
        e[q] = 1e-4 if q < 2 else 1e-2
        vp = eo.sample(img, *eo.warp_sim(p + e, x, y, cx, cy))[1]
        vm = eo.sample(img, *eo.warp_sim(p - e, x, y, cx, cy))[1]
        fd = (vp - vm) / (2 * e[q])
        np.testing.assert_allclose(J[:, q], fd, rtol=1e-6, atol=1e-6 * np.abs(fd).max())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_homography_jacobian_equals_finite_differences(seed):
    rng = np.random.default_rng(seed)
    h, w = 301, 417
    img = _ramp(h, w, *rng.uniform(-3, 3, 2))
    cx, cy = eo.centre(h, w)
    R = eo.norm_radius(h, w)
    th = rng.uniform(-0.05, 0.05)
    hp = np.array([np.cos(th), -np.sin(th), rng.uniform(-0.03, 0.03), np.sin(th), np.cos(th), rng.uniform(-0.03, 0.03),
                   *rng.uniform(-0.02, 0.02, 2)])
    x, y = rng.uniform(40, w - 40, 200), rng.uniform(40, h - 40, 200)
    u, v, den, xn, yn, xp, yp = eo.warp_h(hp, x, y, cx, cy, R)
    valid, _, gx, gy = eo.sample(img, u, v)
    assert valid.all()
    J = eo.jac_h(gx, gy, xn, yn, xp, yp, den, R)
    for q in range(8):
        e = np.zeros(8)
        e[q] = 1e-6
        vp = eo.sample(img, *eo.warp_h(hp + e, x, y, cx, cy, R)[:2])[1]
        vm = eo.sample(img, *eo.warp_h(hp - e, x, y, cx, cy, R)[:2])[1]
        fd = (vp - vm) / 2e-6
        np.testing.assert_allclose(J[:, q], fd, rtol=1e-6, atol=1e-6 * np.abs(fd).max())


def test_sampled_gradient_is_the_interpolated_central_difference():
    """On a quadratic image the central differences are exact at the pixels and the gradient is linear, so its bilinear
    interpolation is the true gradient at any point."""
    rng = np.random.default_rng(5)
    h, w = 60, 80
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c = rng.uniform(-0.05, 0.05, 6)
    img = c[0] * xx * xx + c[1] * xx * yy + c[2] * yy * yy + c[3] * xx + c[4] * yy + c[5]
    u, v = rng.uniform(1, w - 3, 500), rng.uniform(1, h - 3, 500)
    valid, _, gx, gy = eo.sample(img, u, v)
    assert valid.all()
    np.testing.assert_allclose(gx, 2 * c[0] * u + c[1] * v + c[3], rtol=0, atol=1e-9)
    np.testing.assert_allclose(gy, c[1] * u + 2 * c[2] * v + c[4], rtol=0, atol=1e-9)


def test_valid_region_is_the_four_by_four_neighbourhood():
    h, w = 20, 30
    img = np.zeros((h, w))
    u = np.array([0.99, 1.0, w - 2.0 - 1e-9, w - 2.0, 5.0, 5.0, 5.0, 5.0])
    v = np.array([5.0, 5.0, 5.0, 5.0, 0.99, 1.0, h - 2.0 - 1e-9, h - 2.0])
    assert eo.sample(img, u, v)[0].tolist() == [False, True, True, False, False, True, True, False]


# -------------------------------------------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize("shape", [(64, 96), (65, 97), (387, 509), (130, 1031)])
def test_pyramid_levels_are_binomial_blur_then_even_samples(shape):
    from scipy import ndimage
    g = np.random.default_rng(shape[0]).uniform(0, 255, shape)
    k = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]) / 256.0
    lv = eo.pyramid(g, 4)
    want = ndimage.convolve(g, k, mode="nearest")
    np.testing.assert_allclose(lv[0], want, rtol=0, atol=1e-9)
    for lvl in range(1, 4):
        want = ndimage.convolve(want, k, mode="nearest")[::2, ::2]
        assert lv[lvl].shape == ((lv[lvl - 1].shape[0] + 1) // 2, (lv[lvl - 1].shape[1] + 1) // 2)
        np.testing.assert_allclose(lv[lvl], want, rtol=0, atol=1e-9)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_gray_image_of_both_subsampling_rules(dtype):
    rng = np.random.default_rng(3)
    hi = np.iinfo(dtype).max
    img = rng.integers(0, hi + 1, (11, 14, 3)).astype(dtype)
    f = img.astype(np.float64)
    np.testing.assert_allclose(eo.gray(img), 0.114 * f[..., 0] + 0.587 * f[..., 1] + 0.299 * f[..., 2], rtol=1e-15)
    assert eo.gray(img, 3).shape == (4, 5)                           # ceil(11 / 3), ceil(14 / 3)
    np.testing.assert_allclose(eo.gray(img, 3), eo.gray(img[::3, ::3]), rtol=0)
    a = eo.gray(img, 3, area=True)
    assert a.shape == (4, 5)                                         # rint(3.67), rint(4.67)
    # a whole block: round-half-even of the float32 product sum * (1 / 9), per channel
    blk = img[3:6, 6:9].reshape(-1, 3).astype(np.uint32).sum(0)
    c = np.rint(blk.astype(np.float32) * np.float32(1 / 9)).astype(np.float64)
    assert a[1, 2] == pytest.approx(0.114 * c[0] + 0.587 * c[1] + 0.299 * c[2], rel=1e-15)
    # the hanging last row: 11 = 3 * 3 + 2 -> rows 9, 10, mean of the 2 x 3 pixels that exist
    blk = img[9:11, 0:3].reshape(-1, 3).astype(np.uint32).sum(0)
    c = np.rint(blk.astype(np.float32) / np.float32(6)).astype(np.float64)
    assert a[3, 0] == pytest.approx(0.114 * c[0] + 0.587 * c[1] + 0.299 * c[2], rel=1e-15)
    # s = 2: (sum + 2) >> 2
    blk = img[2:4, 4:6].reshape(-1, 3).astype(np.uint32).sum(0)
    c = ((blk + 2) >> 2).astype(np.float64)
    assert eo.gray(img, 2, area=True)[1, 2] == pytest.approx(0.114 * c[0] + 0.587 * c[1] + 0.299 * c[2], rel=1e-15)


# --------------------------------------------------------------------------------------------------------------- tables
# (height, width, s, area) -> the level shapes (finest first) and their sample steps, worked out by hand from the rules:
# halve while the short side of the ceil(dim / s) grid / 2 >= 48 (at most 8 levels); step = largest with
# step^2 * 300000 <= pixels
TABLES = [
    ((4000, 6000, 1, False), [(4000, 6000), (2000, 3000), (1000, 1500), (500, 750), (250, 375), (125, 188), (63, 94)],
     [8, 4, 2, 1, 1, 1, 1]),
    ((4000, 6000, 2, False), [(2000, 3000), (1000, 1500), (500, 750), (250, 375), (125, 188), (63, 94)], [4, 2, 1, 1, 1, 1]),
    ((4000, 6000, 2, True), [(2000, 3000), (1000, 1500), (500, 750), (250, 375), (125, 188), (63, 94)], [4, 2, 1, 1, 1, 1]),
    ((4000, 6000, 4, False), [(1000, 1500), (500, 750), (250, 375), (125, 188), (63, 94)], [2, 1, 1, 1, 1]),
    ((387, 509, 1, False), [(387, 509), (194, 255), (97, 128), (49, 64)], [1, 1, 1, 1]),
    ((387, 509, 2, False), [(194, 255), (97, 128), (49, 64)], [1, 1, 1]),
    ((387, 509, 2, True), [(194, 254), (97, 127), (49, 64)], [1, 1, 1]),       # rint(193.5) = 194, rint(254.5) = 254
    ((130, 1031, 1, False), [(130, 1031), (65, 516)], [1, 1]),
    ((130, 1031, 3, True), [(43, 344)], [1]),
    ((48, 64, 1, False), [(48, 64)], [1]),
]


@pytest.mark.parametrize("key,shapes,steps", TABLES)
def test_level_geometry_and_sample_step_tables(key, shapes, steps):
    h, w, s, area = key
    got = eo.level_shapes(h, w, s, area)
    assert got == shapes
    assert [eo.sample_step(a * b) for a, b in got] == steps
    assert eo.level_shapes(h, w, s, area, max_levels=2) == shapes[:2]


def test_sample_step_boundaries():
    assert eo.sample_step(299999) == 1 and eo.sample_step(1200000) == 2 and eo.sample_step(1199999) == 1
    assert eo.sample_step(24000000) == 8 and eo.sample_step(24300000) == 9
    assert eo.sample_step(24000000, min_samples=200000) == 10


# ------------------------------------------------------------------------------------------------------------- recovery
@pytest.mark.parametrize("theta,s,tx,ty,dtype", [
    (0.5, 1.003, 7.3, -4.6, np.uint8),
    (-0.8, 0.994, -12.4, 9.7, np.uint8),
    (0.02, 1.0001, 0.37, -0.21, np.uint16),
    (1.28, 1.0064, 23.7, -13.4, np.uint8),
])
def test_oracle_recovers_known_similarity(oracle, theta, s, tx, ty, dtype):
    """The similarities of test_gpu_ecc.test_recovers_known_similarity, noise-free: all four corners within 0.02 px."""
    T = similarity(theta, s, tx, ty, 255.5, 255.5)
    ref, mov = make_pair(oracle, T, noise=0.0, dtype=dtype)
    r = eo.estimate(ref, mov)
    assert not r.failed and r.cc > 0.99
    assert eo.corner_deviation(r.M, invert(T), 512, 512) < 0.02, r
    assert len(r.level_iters) == 4 and all(1 <= k <= 60 for k in r.level_iters) and sum(r.level_iters) == r.iters
    # the diagnostics: rho rises on the finest level, the last step's rho is the reported cc
    fine = [st["rho"] for st in r.steps if st["level"] == 0]
    assert len(fine) == r.level_iters[-1] and fine[-1] == r.cc and fine[-1] >= fine[0]


def test_oracle_recovers_a_projective_transform(oracle):
    h, w = 384, 512
    cx, cy = (w - 1) / 2, (h - 1) / 2
    S = np.vstack([similarity(0.4, 1.003, 6.0, -4.0, cx, cy), [0, 0, 1]])
    P = np.array([[1, 0, 0], [0, 1, 0], [4.8e-5, -2.4e-5, 1]])
    C, Ci = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]]), np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
    T = S @ C @ P @ Ci
    T /= T[2, 2]
    base = np.clip(np.repeat(texture(h, w, 17)[:, :, None], 3, 2), 0, 255).astype(np.uint8)
    mov = oracle.warp_perspective(base, T, border_mode=oracle.BORDER_REPLICATE)
    want = np.linalg.inv(T)
    want /= want[2, 2]
    r = eo.estimate(base, mov, homography=True)
    assert r.h_used and r.cc9 >= r.cc
    assert eo.corner_deviation(r.M9, want, h, w) < 0.02 < 1.0 < eo.corner_deviation(r.M, want, h, w), r


def test_refine_from_a_perturbed_start_with_a_third_of_the_frame_outside(oracle):
    T = similarity(0.0, 1.0, 170.0, 0.0, 255.5, 255.5)
    ref, mov = make_pair(oracle, T, noise=0.0)
    m0 = invert(similarity(0.2, 1.0, 172.0, -2.0, 255.5, 255.5))
    for levels in (1, 2):
        r = eo.estimate(ref, mov, M_init=m0, levels=levels)
        assert len(r.level_iters) == levels
        assert eo.corner_deviation(r.M, invert(T), 512, 512) < 0.02, (levels, r)


# ------------------------------------------------------------------------------------------------------------- failures
def test_flat_frame_fails_with_identity_and_cc_minus_two(oracle):
    ref, _ = make_pair(oracle, similarity(0, 1, 0, 0, 63.5, 63.5), h=128, w=128)
    r = eo.estimate(ref, np.full_like(ref, 77))
    assert r.failed and r.cc == -2.0 and np.array_equal(r.M, [[1, 0, 0], [0, 1, 0]])
    assert r.iters == 1 and r.steps[0]["status"] == "fail"
    r = eo.estimate(ref, np.full_like(ref, 77), homography=True)
    assert not r.h_used and r.cc9 == -2.0 and np.array_equal(r.M9, np.eye(3))


def test_start_that_leaves_fewer_than_64_samples_fails(oracle):
    ref, mov = make_pair(oracle, similarity(0, 1, 0, 0, 63.5, 63.5), h=128, w=128)
    m0 = np.array([[1.0, 0.0, 300.0], [0.0, 1.0, 0.0]])            # the moving frame entirely off the template
    r = eo.estimate(ref, mov, M_init=m0, levels=2)
    assert r.failed and r.cc == -2.0 and np.array_equal(r.M, [[1, 0, 0], [0, 1, 0]]) and r.level_iters == [1, 0]


def test_a_frame_registered_against_itself_is_the_identity(oracle):
    ref, _ = make_pair(oracle, similarity(0, 1, 0, 0, 95.5, 63.5), h=128, w=192)
    lv = eo.frame_pyramid(ref)
    r = eo.solve_pyramids(lv, lv)
    assert not r.failed and r.cc == pytest.approx(1.0, abs=1e-12)
    assert eo.corner_deviation(r.M, [[1, 0, 0], [0, 1, 0]], 128, 192) < 1e-9
