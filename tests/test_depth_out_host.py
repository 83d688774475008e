"""CPU: the host side of the depth map output (shinestacker_amd/depth_out.py) and its NumPy restatement
(tests/depth_restatement.py): taps, option checks, the quantiser, the restatement's error against float64 and the semantics
of the confidence-weighted smoothing.  The kernels are held to the restatement in tests/test_gpu_depth_out.py."""
import inspect
import math

import numpy as np
import pytest

import depth_restatement as dr
from shinestacker_amd import InvalidOptionError, depth_out

SIGMAS = (0.3, 0.5, 1.0, 2.0, 2.5, 7.0, 16.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_taps_sum_to_one_are_symmetric_and_span_three_sigma(sigma, dtype):
    k = depth_out.gaussian_taps(sigma, dtype)
    r = math.ceil(3 * sigma)
    assert depth_out.radius_of(sigma) == r and k.dtype == dtype and k.shape == (2 * r + 1,)
    assert np.array_equal(k, k[::-1]) and np.all(k > 0) and k.argmax() == r
    # each tap is rounded once (half an ulp of a value below 1), the float64 quotients before the rounding sum to 1 within
    # one rounding each as well: one eps of the working type per tap covers both
    total = math.fsum(float(v) for v in k)
    assert abs(total - 1.0) <= len(k) * np.finfo(dtype).eps
    # the rule itself, written out once more
    t = [math.exp(-(x * x) / (2.0 * sigma * sigma)) for x in range(-r, r + 1)]
    s = 0.0
    for v in t:
        s += v
    assert np.array_equal(k, np.array([v / s for v in t]).astype(dtype))
    assert np.array_equal(k, dr.taps_of(sigma, dtype))      # the restatement builds the same numbers on its own


def test_largest_sigma_has_radius_48():
    assert depth_out.radius_of(depth_out.MAX_SIGMA) == 48 and len(depth_out.gaussian_taps(16.0)) == 97


@pytest.mark.parametrize("sigma", [0, 0.0, -1.0, 16.0001, 100, float("nan"), float("inf"), "2", None, True])
def test_taps_reject_a_sigma_outside_the_range(sigma):
    with pytest.raises(InvalidOptionError):
        depth_out.gaussian_taps(sigma)


def test_option_checks():
    assert depth_out.check_sigma(0) == 0.0 and depth_out.check_sigma(16) == 16.0 and depth_out.check_sigma(2.0, (7, 7)) == 2.0
    for bad in (-0.5, 16.5, float("nan"), "1", None):
        with pytest.raises(InvalidOptionError):
            depth_out.check_sigma(bad)
    # radius >= min(H, W) is refused, radius = min - 1 is the largest that fits; sigma 0 fits anything
    with pytest.raises(InvalidOptionError):
        depth_out.check_sigma(2.0, (6, 100))
    with pytest.raises(InvalidOptionError):
        depth_out.check_sigma(2.0, (100, 6))
    assert depth_out.check_sigma(0.0, (1, 1)) == 0.0
    with pytest.raises(InvalidOptionError):
        depth_out.gaussian_taps(1.0, np.float16)
    # the binding refuses what needs no device to refuse, before it looks for one
    v, w = np.zeros((8, 9), np.int32), np.ones((8, 9), np.float32)
    for args in ((v, w, 17.0), (v, w, 3.0), (v, w.astype(np.float16), 1.0), (v.astype(np.int64), w, 1.0),
                 (v.astype(np.float64), w, 1.0), (v[:7], w, 1.0), (v[0], w[0], 1.0)):
        with pytest.raises(InvalidOptionError):
            depth_out.weighted_smooth(*args)


def test_quantiser():
    n = 6
    d = np.array([[0.0, n - 1.0, (n - 1) / 2.0, 1.0, (n - 1) * (0.5 / 65535), (n - 1) * (1.5 / 65535)]], np.float32)
    q = depth_out.quantize(d, n)
    assert q.dtype == np.uint16 and q.shape == d.shape
    # 0 -> 0, N - 1 -> 65535, the middle 32767.5 -> 32768 (floor(x + 0.5): halves go up), 1 of 5 -> 13107
    assert q[0, :4].tolist() == [0, 65535, 32768, 13107]
    want = np.floor(d.astype(np.float64) / (n - 1) * 65535.0 + 0.5)
    assert np.array_equal(q, want.astype(np.uint16))
    assert np.array_equal(depth_out.quantize(np.array([[0.0, 3.0]]), 1), np.zeros((1, 2), np.uint16))      # N == 1: all zero
    assert depth_out.quantize(np.array([0.5]), 2)[0] == 32768
    with pytest.raises(InvalidOptionError):
        depth_out.quantize(d, 0)


def test_png_writer_round_trips_16_bit_grey(tmp_path):
    from shinestacker_amd.imageio import read_img
    g = (np.arange(37 * 53, dtype=np.uint32).reshape(37, 53) * 2731 % 65536).astype(np.uint16)
    path = depth_out.save(str(tmp_path / "maps"), "stack_0000", g.astype(np.float64) * (5 / 65535), 6)
    assert path.endswith("maps/stack_0000.png")
    back = read_img(path)
    back = back[:, :, 0] if back.ndim == 3 else back
    assert back.dtype == np.uint16 and np.array_equal(back, depth_out.quantize(g.astype(np.float64) * (5 / 65535), 6))


@pytest.mark.parametrize("sigma,shape", [(0.5, (5, 7)), (2.0, (37, 53)), (16.0, (60, 71))])
def test_float32_restatement_against_float64(sigma, shape):
    """Every term is non-negative, so the first-order error of the float32 evaluation against the float64 one WITH THE SAME
    (float32-rounded) taps is bounded term by term: one rounding for v * w, per pass one for each product and one for each of
    the K partial sums (2 K per pass, 4 K for the numerator; the same for the denominator enters the quotient with the same
    relative size, and the numerator's share is what |D| <= max(v) scales), the divide and the final casts -- in units of
    2^-24 relative to max(v):  |D32 - D64| <= (4 K + 8) * 2^-24 * max(v)."""
    rng = np.random.default_rng(int(sigma * 10) + shape[0])
    K = 2 * dr.radius_of(sigma) + 1
    for vmax, wmax in ((7, 1.0), (255, 4.3e9)):
        v = rng.integers(0, vmax + 1, shape).astype(np.int32)
        w = (rng.random(shape) * wmax).astype(np.float32)
        d32 = dr.weighted_smooth(v, w, sigma, np.float32)
        d64 = dr.weighted_smooth_f64(v, w, sigma, np.float32)
        assert d32.dtype == np.float32 and d64.dtype == np.float64
        err = np.abs(d32.astype(np.float64) - d64).max()
        bound = (4 * K + 8) * 2.0 ** -24 * float(v.max())
        print(f"sigma {sigma} shape {shape} vmax {vmax}: max |D32 - D64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        # a weighted mean stays inside the range of its values (up to the same error)
        assert d32.min() >= v.min() - bound and d32.max() <= v.max() + bound


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_smoothing_semantics(dtype):
    sigma, r = 1.0, 3
    rng = np.random.default_rng(5)
    v = rng.integers(0, 40, (31, 29)).astype(np.int32)
    # all weights zero: the value comes back exactly, everywhere
    out = dr.weighted_smooth(v, np.zeros(v.shape, dtype), sigma, dtype)
    assert out.dtype == np.float32 and np.array_equal(out, v.astype(np.float32))
    # one non-zero weight: its value fills its window, every pixel whose window misses it keeps its own value exactly
    w = np.zeros(v.shape, dtype)
    cy, cx = 15, 12
    w[cy, cx] = 3.5
    out = dr.weighted_smooth(v, w, sigma, dtype)
    yy, xx = np.mgrid[:v.shape[0], :v.shape[1]]
    inside = (np.abs(yy - cy) <= r) & (np.abs(xx - cx) <= r)
    assert np.array_equal(out[~inside], v[~inside].astype(np.float32))
    K = 2 * r + 1
    bound = (4 * K + 8) * 2.0 ** -24 * float(v.max())
    assert np.abs(out[inside].astype(np.float64) - float(v[cy, cx])).max() <= bound
    # sigma 0 is the value itself; uniform weights on a constant plane give the constant back within the bound
    assert np.array_equal(dr.weighted_smooth(v, w, 0, dtype), v.astype(np.float32))
    c = np.full(v.shape, 17, np.int32)
    assert np.abs(dr.weighted_smooth(c, np.ones(v.shape, dtype), 2.0, dtype) - 17.0).max() <= (4 * 13 + 8) * 2.0 ** -24 * 17


def test_depth_index_restatement():
    rng = np.random.default_rng(11)
    planes = rng.random((4, 9, 11)).astype(np.float32)
    planes[:, 2, 3] = 0
    total = planes.sum(0, dtype=np.float32)
    d = dr.depth_index(planes, total)
    assert d.dtype == np.float32 and d[2, 3] == 0
    want = (planes.astype(np.float64) * np.arange(4)[:, None, None]).sum(0) / np.where(total == 0, 1, total)
    # N products, N sums and the divide, each one rounding of a value that D <= N - 1 = 3 bounds: (2 N + 1) * 2^-24 * 3
    assert np.abs(d - want).max() <= (2 * 4 + 1) * 2.0 ** -24 * 3
    assert d.min() >= 0 and d.max() <= 3 * (1 + 2.0 ** -20)
    one = np.zeros((3, 2, 2), np.float64)
    one[2] = 0.25
    assert np.array_equal(dr.depth_index(one, one.sum(0)), np.full((2, 2), 2.0))


def test_public_surface_has_defaults():
    import shinestacker_amd as sa
    from shinestacker_amd import pipeline
    assert sa.depth_out is depth_out and "depth_out" in sa.__all__
    assert inspect.signature(sa.PyramidStack.depth_map).parameters["sigma"].default == 2.0
    assert inspect.signature(sa.DepthMapStack.depth_map).parameters["sigma"].default == 0.0
    for fn in (pipeline.align_and_stack, pipeline.align_and_stack_device):
        assert inspect.signature(fn).parameters["depth_map"].default is None
    assert inspect.signature(depth_out.weighted_smooth).parameters["device"].default == 0
    with pytest.raises(RuntimeError):
        sa.PyramidStack().depth_map()
    with pytest.raises(RuntimeError):
        sa.DepthMapStack().depth_map()
    # the option is refused before anything is allocated
    with pytest.raises(InvalidOptionError):
        pipeline._check_depth_map(2.0, None, (64, 64))
    with pytest.raises(InvalidOptionError):
        pipeline._check_depth_map(20.0, {}, (64, 64))
    assert pipeline._check_depth_map(None, None, (64, 64)) is None and pipeline._check_depth_map(True, {}, (64, 64)) == 2.0
