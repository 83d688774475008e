"""GPU: the post-stack denoise (csrc/kernels_denoise.hpp) and the unsharp mask (csrc/kernels_unsharp.hpp) against their NumPy
restatements on the cases of tests/poststack_cases.py -- every template half size 0..5 and search half sizes 0, 1, 5, 10, the
weight table in LDS (up to the largest request, 63 644 bytes) and in global memory (up to the whole 195 076-entry table), frames
of one row, one column and one pixel, frames that end on a tile edge and one pixel past it, saturated frames that put the
accumulators at their bounds; unsharp windows 1 to 25 (uint8) and 1 to 33 (uint16) in both branches.  Every comparison is array_equal.
test_poststack_cases_host.py checks on the CPU that the restatement moves enough of every case for the comparison to mean
something; test_gpu_denoise.py and test_gpu_retouch.py replay the recorded fixtures."""
import numpy as np
import pytest

import poststack_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hiplib):
    hiplib.require_device()
    return hiplib


def through_device(lib, img, run):
    """`run(src, dst)` on device buffers: (what it wrote, the source afterwards)"""
    buffers = []
    try:
        for _ in range(2):
            buffers.append(lib.DeviceBuffer(img.nbytes))
        src, dst = buffers
        src.upload(img)
        dst.upload(~img)            # whatever the kernel does not write stays wrong
        run(src.ptr, dst.ptr)
        lib.check(lib.load().mi_device_synchronize(0))
        return dst.download(img.shape, img.dtype), src.download(img.shape, img.dtype)
    finally:
        for b in buffers:
            b.free()


def assert_same(name, got, want, img, identity):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:5])
    if identity:
        assert np.array_equal(got, img), (name, "a declared identity", int((got != img).sum()))


# ---------------------------------------------------------------- denoise
def denoise_goes_through_device(c):
    """the largest LDS request, one global-table case per dtype, and the whole table without a zero entry"""
    key = (c.dtype, c.h, c.template, c.search)
    return c.group == "placement" and key in (pc.LARGEST_LDS, (np.uint8, 100, 1, 21), (np.uint16, 10, 7, 21))


@pytest.mark.parametrize("group", pc.DENOISE_GROUPS)
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_denoise_equals_the_restatement(dev, dtype, group):
    from shinestacker_amd import denoise
    from shinestacker_amd.denoise import denoise_device
    cases = [c for c in pc.DENOISE_CASES if c.dtype == dtype and c.group == group]
    assert cases
    for c in cases:
        img, want, name = pc.denoise_frame(c), pc.denoise_expected(c), pc.denoise_name(c)
        assert_same(name, denoise(img, c.h, c.template, c.search), want, img, c.identity)
        if denoise_goes_through_device(c):
            h, w = c.shape
            got, src_after = through_device(dev, img, lambda s, d: denoise_device(s, d, h, w, img.dtype, c.h, c.template, c.search))
            assert_same((name, "device entry point"), got, want, img, c.identity)
            assert np.array_equal(src_after, img), (name, "the source moved")
    if group == "placement":
        assert sum(denoise_goes_through_device(c) for c in cases) == (4 if dtype == np.uint8 else 2)


# ---------------------------------------------------------------- unsharp
def unsharp_goes_through_device(c):
    """constant(max) on 33 x 65 at radius 4, both branches (uint16: both halves of the split column sum at their largest)"""
    return (c.group, c.kind, c.shape, c.radius) == ("extreme", "constant", (33, 65), 4)


@pytest.mark.parametrize("group", pc.UNSHARP_GROUPS)
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_unsharp_mask_equals_the_restatement(dev, dtype, group):
    from shinestacker_amd import unsharp_mask
    from shinestacker_amd.sharpen import unsharp_mask_device
    cases = [c for c in pc.UNSHARP_CASES if c.dtype == dtype and c.group == group]
    assert cases
    for c in cases:
        img, want, name = pc.unsharp_frame(c), pc.unsharp_expected(c), pc.unsharp_name(c)
        assert_same(name, unsharp_mask(img, c.radius, c.amount, c.threshold), want, img, c.identity)
        if unsharp_goes_through_device(c):
            h, w = c.shape
            got, src_after = through_device(dev, img, lambda s, d: unsharp_mask_device(s, d, h, w, img.dtype, c.radius, c.amount,
                                                                                      c.threshold))
            assert_same((name, "device entry point"), got, want, img, c.identity)
            assert np.array_equal(src_after, img), (name, "the source moved")
    if group == "extreme":
        assert sum(unsharp_goes_through_device(c) for c in cases) == 2
