"""The reference's unsharp mask (algorithms/sharpen.py) restated in NumPy on top of oracle.gaussian_blur_fixed.

    blurred = cv2.GaussianBlur(image, (0, 0), radius)
    threshold == 0:  cv2.addWeighted(image, 1 + amount, blurred, -amount, 0)
    threshold != 0:  the reference's own NumPy lines (threshold * 256 for uint16)

The two cv2 primitives are OpenCV's rules as remembered [from memory, unpinned: no OpenCV was at hand when this was written]:

    GaussianBlur with ksize (0, 0): ksize = cvRound(sigma * 6 + 1) | 1 for 8-bit, cvRound(sigma * 8 + 1) | 1 for 16-bit
        (cvRound: half to even on the double), then the bit-exact fixed-point path oracle/align_oracle.c states
    addWeighted on 8- / 16-bit frames: float32 -- alpha = f32(1 + amount), beta = f32(-amount), each product rounded to
        float32, their sum rounded to float32 (no fused multiply-add), cvRound (half to even), saturated

The thresholded branch is the reference's code, pinned by the recorded fixtures (tools/gen_golden_retouch.py).  Written for
the tests and the fixture recorder; it shares nothing with shinestacker_amd/sharpen.py or the kernel.
"""
import numpy as np


def window_size(dtype, sigma):
    """the window cv2.GaussianBlur derives from sigma when ksize is (0, 0)"""
    return int(np.rint(np.float64(sigma) * (6 if np.dtype(dtype) == np.uint8 else 8) + 1)) | 1     # rint: half to even


def gaussian_blur(image, ksize, sigma):
    """cv2.GaussianBlur(image, ksize, sigma) for 8- / 16-bit frames; ksize (0, 0) is derived from sigma"""
    from oracle import oracle as orc
    assert ksize[0] == ksize[1] and image.dtype in (np.uint8, np.uint16) and sigma > 0
    k = ksize[0] if ksize[0] > 0 else window_size(image.dtype, sigma)
    return orc.gaussian_blur_fixed(image, k, sigma)


def add_weighted(src1, alpha, src2, beta, gamma):
    """cv2.addWeighted for 8- / 16-bit frames: float32 products and sum, half to even, saturated"""
    assert src1.dtype == src2.dtype and src1.dtype in (np.uint8, np.uint16) and gamma == 0
    a, b = np.float32(alpha), np.float32(beta)
    t1 = (src1.astype(np.float32) * a).astype(np.float32)
    t2 = (src2.astype(np.float32) * b).astype(np.float32)
    s = (t1 + t2).astype(np.float32)
    return np.clip(np.rint(s), 0, np.iinfo(src1.dtype).max).astype(src1.dtype)


def unsharp_mask(image, radius=1.0, amount=1.0, threshold=0.0):
    """sharpen.py:6-22 for uint8 / uint16 frames"""
    assert image.dtype in (np.uint8, np.uint16)
    if image.dtype == np.uint16:
        threshold = threshold * 256
    blurred = gaussian_blur(image, (0, 0), radius)
    if threshold == 0:
        return add_weighted(image, 1.0 + amount, blurred, -amount, 0)
    fi, fb = image.astype(np.float32), blurred.astype(np.float32)
    diff = fi - fb
    mask = np.abs(diff) > np.float32(threshold)
    val = (fi + (np.float32(amount) * diff).astype(np.float32)).astype(np.float32)
    out = np.clip(np.where(mask, val, fi), 0, np.iinfo(image.dtype).max)
    return out.astype(image.dtype)      # truncation toward zero
