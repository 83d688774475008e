"""Synthetic registration pairs shared by the estimator tests (tests/test_gpu_ecc.py, tests/test_ecc_oracle.py,
tests/test_gpu_ecc_oracle.py and the alignment tests that import them from test_gpu_ecc): a textured gray scene with
hard-edged shapes, the similarity / perspective that moves it, and the moving frame made by the oracle's warp."""
import numpy as np


def texture(h, w, seed):
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.float64)
    for sigma, amp in ((1.5, 60), (4, 50), (12, 40)):
        img += amp * ndimage.gaussian_filter(rng.standard_normal((h, w)), sigma) * sigma
    img = 128 + img * (60 / img.std())
    # a few hard-edged shapes, as in the reference's synthetic test image
    yy, xx = np.mgrid[0:h, 0:w]
    img[(yy - h * 0.3) ** 2 + (xx - w * 0.6) ** 2 < (0.08 * h) ** 2] += 70
    img[int(h * 0.55):int(h * 0.8), int(w * 0.15):int(w * 0.4)] -= 60
    return np.clip(img, 0, 255)


def similarity(theta_deg, s, tx, ty, cx, cy):
    t = np.deg2rad(theta_deg)
    a, b = s * np.cos(t), s * np.sin(t)
    return np.array([[a, -b, cx - a * cx + b * cy + tx], [b, a, cy - b * cx - a * cy + ty]])


def invert(M):
    A = M[:, :2]
    Ai = np.linalg.inv(A)
    return np.hstack([Ai, -Ai @ M[:, 2:3]])


def decompose(M):
    s = np.hypot(M[0, 0], M[1, 0])
    return np.rad2deg(np.arctan2(M[1, 0], M[0, 0])), s, M[0, 2], M[1, 2]


def make_pair(oracle, T, h=512, w=512, noise=5.0, seed=0, dtype=np.uint8):
    rng = np.random.default_rng(seed + 100)
    base = texture(h, w, seed)
    scale = 1 if dtype == np.uint8 else 257
    ref3 = np.repeat(base[:, :, None], 3, 2)
    mov3 = oracle.warp_affine(np.clip(ref3, 0, 255).astype(np.uint8), T, border_mode=oracle.BORDER_REPLICATE)
    ref = np.clip(ref3 + rng.normal(0, noise, ref3.shape), 0, 255)
    mov = np.clip(mov3.astype(np.float64) + rng.normal(0, noise, ref3.shape), 0, 255)
    return (ref * scale).astype(dtype), (mov * scale).astype(dtype)
