"""GPU: the alignment apply step (csrc/kernels_align.hpp, warp_launch / blur_launch / warp_device_impl in csrc/capi.hip)
against oracle/align_oracle.c on the cases of tests/warp_cases.py -- every tile path of the warp kernel (staged through LDS,
the LDS-budget and buffer-end fallbacks, per-pixel tiles of both thread-row kinds, ring and no ring), frames on the tile grid
and one row past it, frames of one row, one column, one pixel and below the blur radius, reflections, quarter and half turns,
2x zooms, singular matrices, saturated frames, blur kernels 1 .. 31, more blur tiles than the blur grid has workgroups, the
homography's block edges and a horizon inside the frame; the device entry points with unaligned pointers and guard bands; the
per-stream scratch after a larger frame.  Every comparison is array_equal, mask included.  test_warp_cases_host.py checks on
the CPU that every case reaches what it is there for; test_gpu_align.py holds the first rounds' inputs."""
import ctypes as C

import numpy as np
import pytest

import warp_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


def assert_same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError((name, "%d of %d differ" % (len(bad), want.size), bad[:5].tolist()))


def run_case(L, c):
    fn = L.warp_perspective if c.kind == "perspective" else L.warp_affine
    img, M = wc.frame_of(c), wc.matrix_of(c)
    for mode, ks, sigma in wc.runs_of(c):
        name = (wc.case_name(c), "mode %d" % mode, "blur (%d, %g)" % (ks, sigma))
        want, wmask = wc.expected(c, mode, ks, sigma)
        got, gmask = fn(img, M, border_mode=mode, border_value=wc.border_value(c.dtype), blur_ksize=ks, blur_sigma=sigma,
                        want_mask=True)
        assert_same(name + ("mask",), gmask, wmask)
        assert_same(name + ("image",), got, want)


@pytest.mark.parametrize("group", wc.GROUPS)
@pytest.mark.parametrize("dtype", wc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_warp_equals_the_oracle(L, dtype, group):
    cases = wc.cases_of(group, dtype)
    assert cases
    for c in cases:
        run_case(L, c)


# ---------------------------------------------------------------- the device entry points
GUARD = 64            # preset bytes in front of and behind every placed buffer
GUARD_BYTE, TMP_BYTE, MASK_BYTE = 0x5A, 0xA5, 0xEE


class Placed:
    """`content` at `offset` bytes past a 64-byte boundary of a device buffer, 64 guard bytes on either side"""

    def __init__(self, lib, content, offset):
        self.content = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
        self.lo = GUARD + offset
        self.image = np.full(self.lo + self.content.size + GUARD, GUARD_BYTE, np.uint8)
        self.image[self.lo:self.lo + self.content.size] = self.content
        self.buf = lib.DeviceBuffer(self.image.size)
        assert self.buf.ptr % 64 == 0
        self.buf.upload(self.image)
        self.ptr = self.buf.ptr + self.lo

    def read(self, shape, dtype):
        """(what lies at the placement now, the guard bands are as they were)"""
        now = self.buf.download(self.image.shape, np.uint8)
        hi = self.lo + self.content.size
        intact = np.array_equal(now[:self.lo], self.image[:self.lo]) and np.array_equal(now[hi:], self.image[hi:])
        return now[self.lo:hi].copy().view(dtype).reshape(shape), intact

    def free(self):
        self.buf.free()


def through_device(L, fn, img, M, mode, ks, sigma, want, wmask, src_off=0, dst_off=0, mask_off=0, no_mask=False):
    """one call of a device entry point with dst, tmp and mask preset to wrong patterns"""
    h, w = img.shape[:2]
    placed = []
    try:
        src = Placed(L, img, src_off)
        placed.append(src)
        dst = Placed(L, ~want, dst_off)         # whatever the kernel does not write stays wrong
        placed.append(dst)
        tmp = mask = None
        if not no_mask:
            tmp = Placed(L, np.full(img.nbytes, TMP_BYTE, np.uint8), 0)
            placed.append(tmp)
            mask = Placed(L, np.full(h * w, MASK_BYTE, np.uint8), mask_off)
            placed.append(mask)
        m = (C.c_double * M.size)(*M.reshape(-1))
        bv = (C.c_double * 4)(*wc.border_value(img.dtype))
        L.check(fn(0, None, src.ptr, dst.ptr, tmp.ptr if tmp else None, mask.ptr if mask else None, h, w,
                   L.DTYPE_CODE[np.dtype(img.dtype)], m, mode, bv, ks, sigma))
        L.check(L.load().mi_device_synchronize(0))
        got, dst_guards = dst.read(img.shape, img.dtype)
        src_after, src_guards = src.read(img.shape, img.dtype)
        gmask, mask_guards = mask.read((h, w), np.uint8) if mask else (None, True)
        tmp_guards = tmp.read(img.shape, img.dtype)[1] if tmp else True
        return got, gmask, src_after, (dst_guards, mask_guards, src_guards, tmp_guards)
    finally:
        for p in placed:
            p.free()


def placements(dtype):
    """(name, keyword arguments): byte offsets from a 64-byte boundary; a uint16 pointer stays 2-byte aligned, so its
    `+ 1` and `+ 3` are in samples (2 and 6 bytes: no 4-byte boundary either)"""
    e = np.dtype(dtype).itemsize
    out = [("aligned", {}), ("mask + 1", {"mask_off": 1}), ("mask + 3", {"mask_off": 3}),
           ("src + 1", {"src_off": 1 * e}), ("src + 3", {"src_off": 3 * e}),
           ("dst + 1" if e == 1 else "dst + 2", {"dst_off": 1 if e == 1 else 2})]
    return out


@pytest.mark.parametrize("kind", ["affine", "perspective"])
@pytest.mark.parametrize("dtype", wc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_device_entry_with_unaligned_pointers_and_guard_bands(L, dtype, kind):
    lib = L.load()
    fn = lib.mi_warp_perspective_device if kind == "perspective" else lib.mi_warp_affine_device
    img = wc.device_frame(dtype)
    for tname, M2 in wc.DEVICE_TRANSFORMS:
        M = np.array(wc.as_3x3(M2) if kind == "perspective" else M2, np.float64)
        for pname, kw in placements(dtype):
            name = (kind, np.dtype(dtype).name, tname, pname)
            want, wmask = wc.oracle_warp(kind, img, M, 2, *wc.DEVICE_BLUR)
            got, gmask, src_after, guards = through_device(L, fn, img, M, 2, *wc.DEVICE_BLUR, want, wmask, **kw)
            assert_same(name + ("mask",), gmask, wmask)
            assert_same(name + ("image",), got, want)
            assert np.array_equal(src_after, img), (name, "the source moved")
            assert guards == (True, True, True, True), (name, "guard bands (dst, mask, src, tmp)", guards)
        for mode in (0, 1):
            name = (kind, np.dtype(dtype).name, tname, "no mask, no tmp", "mode %d" % mode)
            want, wmask = wc.oracle_warp(kind, img, M, mode)
            got, _none, src_after, guards = through_device(L, fn, img, M, mode, *wc.DEVICE_BLUR, want, wmask, no_mask=True)
            assert_same(name + ("image",), got, want)
            assert np.array_equal(src_after, img), (name, "the source moved")
            assert guards == (True, True, True, True), (name, "guard bands", guards)


# ---------------------------------------------------------------- the per-stream scratch
@pytest.mark.parametrize("dtype", wc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_scratch_serves_a_small_frame_after_a_large_one(L, dtype):
    """the tile scratch and the coordinate table are cached per stream and only grow: a small frame after a large one works
    with the large one's buffers, and the first frame again with what the others left in them"""
    for step, (kind, img, M, ks, sigma) in enumerate(wc.scratch_sequence(dtype)):
        fn = L.warp_perspective if kind == "perspective" else L.warp_affine
        name = ("step %d" % step, kind, img.shape, np.dtype(dtype).name)
        want, wmask = wc.oracle_warp(kind, img, M, 2, ks, sigma)
        got, gmask = fn(img, M, border_mode=2, border_value=wc.border_value(dtype), blur_ksize=ks, blur_sigma=sigma, want_mask=True)
        assert_same(name + ("mask",), gmask, wmask)
        assert_same(name + ("image",), got, want)
