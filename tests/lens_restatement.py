"""The lens remap (csrc/kernels_lens.hpp; include/mi355stack.h, mi_lens_remap) stated in NumPy: the specification the kernel
is held to bit for bit.  Nothing here imports the package.

A lens is 12 finite float64 k[c][0..3], c in B, G, R order like the frames, and a centre (cx, cy) in pixels (default: the
middle of the frame; |cx|, |cy| <= 2^30 -- the library refuses others -- so that cx + (x - cx) is x to far below 1/64 pixel
and a plane of (1, 0, 0, 0), which the kernel copies, is a copy here too).  For the destination pixel (x, y), every step float64 and every operation rounded once -- NumPy's
element-wise operators are exactly that, one IEEE operation each:

    1. dx = x - cx, dy = y - cy
    2. R2 = the largest dx*dx + dy*dy over the four corner pixels
    3. inv = 1.0 / R2, or 0.0 when R2 == 0
    4. u = (dx*dx + dy*dy) * inv
    5. per plane, s = ((k3*u + k2)*u + k1)*u + k0
    6. px = min(max(cx + dx*s, -1.0), w), py = min(max(cy + dy*s, -1.0), h)
    7. X = (int)rint(px * 32), Y = (int)rint(py * 32): positions in 1/32 pixel
    8. sx = X >> 5, fx = X & 31, and the same for y
    9. taps (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1), indices clamped to the frame: v00, v01, v10, v11
   10. out = (v00*(32-fx)*(32-fy) + v01*fx*(32-fy) + v10*(32-fx)*fy + v11*fx*fy + 512) >> 10

The mask is 1 where 0 <= X <= 32 (w - 1) and 0 <= Y <= 32 (h - 1) for all three planes, else 0."""
import numpy as np

IDENTITY = (1.0, 0.0, 0.0, 0.0)


def default_centre(h, w):
    return ((w - 1) / 2.0, (h - 1) / 2.0)


def planes(k):
    """3 x 4 float64 from one plane's (k0, k1, k2, k3) or three (B, G, R)"""
    k = np.asarray(k, np.float64)
    if k.shape == (4,):
        k = np.broadcast_to(k, (3, 4))
    assert k.shape == (3, 4) and np.isfinite(k).all()
    return k


def inv_r2(h, w, cx, cy):
    """steps 2 and 3"""
    cx, cy = np.float64(cx), np.float64(cy)
    r2 = np.float64(0.0)
    for y in (0, h - 1):
        for x in (0, w - 1):
            dx, dy = np.float64(x) - cx, np.float64(y) - cy
            r2 = max(r2, dx * dx + dy * dy)
    return np.float64(0.0) if r2 == 0 else np.float64(1.0) / r2


def positions(h, w, k4, centre=None):
    """steps 1 to 7 for one plane: (X, Y), int64 h x w"""
    cx, cy = (np.float64(v) for v in (default_centre(h, w) if centre is None else centre))
    k0, k1, k2, k3 = (np.float64(v) for v in k4)
    y, x = np.indices((h, w)).astype(np.float64)
    dx, dy = x - cx, y - cy
    u = (dx * dx + dy * dy) * inv_r2(h, w, cx, cy)
    with np.errstate(over="ignore", invalid="ignore"):
        s = ((k3 * u + k2) * u + k1) * u + k0
        # fmax / fmin as C's: a NaN operand (coefficients near the end of the float64 range) gives the other one
        px = np.fmin(np.fmax(cx + dx * s, -1.0), np.float64(w))
        py = np.fmin(np.fmax(cy + dy * s, -1.0), np.float64(h))
    return np.rint(px * 32.0).astype(np.int64), np.rint(py * 32.0).astype(np.int64)


def remap(frame, k, centre=None, return_mask=False):
    """H x W x 3 uint8 / uint16 -> the remapped frame (and the H x W uint8 mask)"""
    frame = np.asarray(frame)
    assert frame.ndim == 3 and frame.shape[2] == 3 and frame.dtype in (np.uint8, np.uint16)
    h, w = frame.shape[:2]
    k = planes(k)
    out = np.empty_like(frame)
    mask = np.ones((h, w), bool)
    for c in range(3):
        X, Y = positions(h, w, k[c], centre)
        mask &= (X >= 0) & (X <= 32 * (w - 1)) & (Y >= 0) & (Y <= 32 * (h - 1))
        sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
        x0, x1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1)
        y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
        v = frame[:, :, c].astype(np.int64)
        acc = v[y0, x0] * (32 - fx) * (32 - fy) + v[y0, x1] * fx * (32 - fy) + v[y1, x0] * (32 - fx) * fy + v[y1, x1] * fx * fy
        out[:, :, c] = ((acc + 512) >> 10).astype(frame.dtype)
    return (out, mask.astype(np.uint8)) if return_mask else out


def scaled(k, f):
    """all 12 coefficients times f"""
    return planes(k) * np.float64(f)
