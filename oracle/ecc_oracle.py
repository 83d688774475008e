"""oracle/ecc_oracle.py -- the ECC transform estimator (csrc/kernels_ecc.hpp, aligner_solve in csrc/capi.hip) restated in
float64 NumPy from its documented algorithm.

TEST INFRASTRUCTURE ONLY: it does not import shinestacker_amd.  The device works in float32 where this module works in
float64 (gray image, pyramid, sample positions, interpolation) and solves its 4 x 4 / 8 x 8 systems by its own
elimination where this module calls np.linalg.solve, so the two agree to the float32 floor of the device, not bit for bit
(tests/test_gpu_ecc_oracle.py states the tolerances).

The algorithm, step by step:

* gray image: 0.114 B + 0.587 G + 0.299 R of the sub-sampled frame -- img[::s, ::s] (grid ceil(dim / s)), or the
  integer-factor INTER_AREA mean (oracle.resize_area_int, grid round-half-even(dim / s));
* pyramid: level 0 = the gray image under the 5 x 5 binomial blur ([1 4 6 4 1] / 16 separable, replicate border); level
  l + 1 = the blur of level l at its even indices ((n + 1) // 2 samples per side).  Levels: halve while the short side of
  the create-time grid (ceil(dim / s)) / 2 >= 48, at most 8 or `max_levels`; their sizes follow the grid in force;
* warp, in coordinates centred on the level's centre c = ((w - 1) / 2, (h - 1) / 2):
  W(x) = c + [a -b; b a](x - c) + t, reference pixel -> position in the moving frame;
* samples: every `step`-th row and column of the reference level (step = the largest with step^2 * 300000 <= pixels, at
  least 1); a sample counts when the 4 x 4 neighbourhood of its position lies inside the moving level
  (1 <= floor(u) <= w - 3, the same for v); the moving level is sampled bilinearly, its gradient is the bilinear
  interpolation of the central differences 0.5 (right - left), 0.5 (below - above);
* one forward-additive step from those samples: rho, the projections ip = J^T (iw - mean), tp = J^T (ir - mean), H = J^T J,
  lambda = (|iw'|^2 - ip H^-1 ip) / (corr - tp H^-1 ip), dp = H^-1 (lambda tp - ip).  Fewer than 64 samples or a constant
  image: the frame FAILS (identity, cc = -2).  A singular H or lambda's denominator <= 0: the level stops, p unchanged.
  The level also stops when the step moves the level's corners by less than 2e-3 px ((|da| + |db|) * |c| + |dtx| + |dty|)
  or when |rho - rho of the previous step| < eps; at most `max_iters` steps per level;
* between levels: T = t + c - A c (origin coordinates), doubled on the way to the next finer level; t = T - c + A c on it;
* read-out: M = W^-1 (moving -> reference) with the translation times s; cc = rho at the START of the last step taken;
* refine: the iteration starts on level levels - 1 (clamped to the pyramid) from W = M_init^-1, T = its translation
  / (s * 2^level);
* pairs: each frame registered against the pyramid of another frame of the batch (itself: the identity, cc = 1);
* homography: from the finest level's similarity, 8 parameters in normalised centred coordinates (xn = (x - c) / R,
  R = float32 hypot(cx, cy)), xn' = (h0 xn + h1 yn + h2) / (h6 xn + h7 yn + 1), ...; a sample needs that denominator
  > 1e-3; stop when sum |dh| * R < 2e-3 or rho stalls.  The 3 x 3 result is kept only when the refinement did not fail,
  took a step, and its rho (again that of the last step's start) is >= the similarity's rho - 1e-9; else the similarity.
"""
import math

import numpy as np

from oracle.oracle import resize_area_int

MIN_SAMPLES = 300000      # samples per sum at least (ecc_sample_step)
MIN_COUNT = 64            # fewer valid samples: the frame fails
STOP_MOVE = 2e-3          # px on the level
MAX_LEVELS = 8
MIN_SHORT = 48            # a level is halved while its short side / 2 >= this


# ---------------------------------------------------------------------------------------------------------------- images
def grid_shape(height, width, s=1, area=False):
    """The sub-sampled grid: ceil(dim / s) (fast), round-half-even(dim / s) (area)."""
    if area and s > 1:
        return int(np.rint(height / s)), int(np.rint(width / s))
    return -(-height // s), -(-width // s)


def gray(img, s=1, area=False):
    """float64 gray image of an H x W x 3 BGR u8 / u16 frame, sub-sampled by s."""
    if s > 1:
        img = resize_area_int(img, s) if area else img[::s, ::s]
    f = img.astype(np.float64)
    return 0.114 * f[..., 0] + 0.587 * f[..., 1] + 0.299 * f[..., 2]


def level_shapes(height, width, s=1, area=False, max_levels=0):
    """[(h, w)] of the pyramid levels, finest first."""
    h, w = grid_shape(height, width, s, False)
    n = 0
    while True:
        n += 1
        if n >= (max_levels if max_levels > 0 else MAX_LEVELS) or min(h, w) // 2 < MIN_SHORT:
            break
        h, w = (h + 1) // 2, (w + 1) // 2
    h, w = grid_shape(height, width, s, area)
    out = []
    for _ in range(n):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


_K5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def blur5(img):
    """5 x 5 binomial blur, replicate border."""
    p = np.pad(img, 2, mode="edge")
    h, w = img.shape
    rows = sum(_K5[t] * p[:, t:t + w] for t in range(5))
    return sum(_K5[t] * rows[t:t + h, :] for t in range(5))


def pyramid(g, nlevels):
    """Level 0 = blur5(gray); level l + 1 = blur5(level l)[::2, ::2]."""
    lv = [blur5(g)]
    for _ in range(1, nlevels):
        lv.append(blur5(lv[-1])[::2, ::2])
    return lv


def frame_pyramid(img, s=1, area=False, max_levels=0):
    shapes = level_shapes(img.shape[0], img.shape[1], s, area, max_levels)
    lv = pyramid(gray(img, s, area), len(shapes))
    assert [x.shape for x in lv] == shapes
    return lv


def sample_step(npix, min_samples=MIN_SAMPLES):
    step = 1
    while (step + 1) ** 2 * min_samples <= npix:
        step += 1
    return step


# ------------------------------------------------------------------------------------------------- warps and sampling
def centre(h, w):
    return 0.5 * (w - 1), 0.5 * (h - 1)


def norm_radius(h, w):
    """The homography's normalisation radius: half the level's diagonal, as the device's float32 hypotf gives it."""
    cx, cy = centre(h, w)
    return float(np.float32(math.hypot(float(np.float32(cx)), float(np.float32(cy)))))


def warp_sim(p, x, y, cx, cy):
    a, b, tx, ty = p
    xc, yc = x - cx, y - cy
    return cx + a * xc - b * yc + tx, cy + b * xc + a * yc + ty


def jac_sim(gx, gy, x, y, cx, cy):
    """d I(W(x; p)) / d(a, b, tx, ty) from the image gradient (gx, gy) at W(x)."""
    xc, yc = x - cx, y - cy
    return np.stack([gx * xc + gy * yc, -gx * yc + gy * xc, gx, gy], axis=-1)


def warp_h(hp, x, y, cx, cy, R):
    """-> (u, v, den, xn, yn, xp, yp)"""
    xn, yn = (x - cx) / R, (y - cy) / R
    den = hp[6] * xn + hp[7] * yn + 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        xp = (hp[0] * xn + hp[1] * yn + hp[2]) / den
        yp = (hp[3] * xn + hp[4] * yn + hp[5]) / den
    return cx + R * xp, cy + R * yp, den, xn, yn, xp, yp


def jac_h(gx, gy, xn, yn, xp, yp, den, R):
    """d I(W(x; h)) / d h for the 8 normalised parameters, (gx, gy) the gradient in pixels at W(x)."""
    gxn, gyn = gx * R / den, gy * R / den
    pr = -(gx * xp + gy * yp) * R / den
    return np.stack([gxn * xn, gxn * yn, gxn, gyn * xn, gyn * yn, gyn, pr * xn, pr * yn], axis=-1)


def sample(img, u, v):
    """Bilinear sample and gradient of `img` at (u, v).  -> (valid, value, gx, gy); the last three only where valid."""
    h, w = img.shape
    fu, fv = np.floor(u), np.floor(v)
    ok = np.isfinite(u) & np.isfinite(v)
    valid = ok & (fu >= 1) & (fv >= 1) & (fu <= w - 3) & (fv <= h - 3)
    x0, y0 = fu[valid].astype(np.int64), fv[valid].astype(np.int64)
    fx, fy = u[valid] - x0, v[valid] - y0

    def bil(f00, f01, f10, f11):
        top = f00 + fx * (f01 - f00)
        bot = f10 + fx * (f11 - f10)
        return top + fy * (bot - top)

    def at(dy, dx):
        return img[y0 + dy, x0 + dx]

    val = bil(at(0, 0), at(0, 1), at(1, 0), at(1, 1))

    def cdx(dy, dx):
        return 0.5 * (at(dy, dx + 1) - at(dy, dx - 1))

    def cdy(dy, dx):
        return 0.5 * (at(dy + 1, dx) - at(dy - 1, dx))

    gx = bil(cdx(0, 0), cdx(0, 1), cdx(1, 0), cdx(1, 1))
    gy = bil(cdy(0, 0), cdy(0, 1), cdy(1, 0), cdy(1, 1))
    return valid, val, gx, gy


def sample_grid(h, w, step):
    ys, xs = np.meshgrid(np.arange(0, h, step, dtype=np.float64), np.arange(0, w, step, dtype=np.float64), indexing="ij")
    return xs.ravel(), ys.ravel()


# ------------------------------------------------------------------------------------------------------ one ECC step
def solve_sym(H, r):
    """H^-1 r for the symmetric positive H; None when H is not positive on the diagonal or (numerically) singular."""
    d = np.diag(H)
    if not np.all(d > 0):
        return None
    sc = 1.0 / np.sqrt(d)
    A = H * sc[:, None] * sc[None, :]
    if not np.isfinite(A).all() or np.linalg.cond(A) > 1e12:
        return None
    try:
        return sc * np.linalg.solve(A, sc * r)
    except np.linalg.LinAlgError:
        return None


def ecc_step(iw, ir, J):
    """The forward-additive ECC step from the valid samples.  -> (status, rho, dp): status 'fail' (frame fails: too few
    samples or a constant image), 'stop' (singular system or lambda's denominator <= 0: rho is set, no step) or 'ok'."""
    n = iw.size
    if n < MIN_COUNT:
        return "fail", None, None
    zw, zr = iw - iw.mean(), ir - ir.mean()
    wn2, rn2, corr = zw @ zw, zr @ zr, zw @ zr
    if not (wn2 > 0) or not (rn2 > 0):
        return "fail", None, None
    rho = corr / math.sqrt(wn2 * rn2)
    ip, tp, H = J.T @ zw, J.T @ zr, J.T @ J
    hi = solve_sym(H, ip)
    if hi is None:
        return "stop", rho, None
    lam_d = corr - tp @ hi
    if not (lam_d > 0):
        return "stop", rho, None
    lam = (wn2 - ip @ hi) / lam_d
    dp = solve_sym(H, lam * tp - ip)
    if dp is None:
        return "stop", rho, None
    return "ok", rho, dp


def sim_terms(tmpl, img, p, step):
    """(iw, ir, J) of the similarity p = (a, b, tx, ty) on one level."""
    h, w = tmpl.shape
    cx, cy = centre(h, w)
    x, y = sample_grid(h, w, step)
    u, v = warp_sim(p, x, y, cx, cy)
    valid, iw, gx, gy = sample(img, u, v)
    ir = tmpl[y[valid].astype(np.int64), x[valid].astype(np.int64)]
    return iw, ir, jac_sim(gx, gy, x[valid], y[valid], cx, cy)


def h_terms(tmpl, img, hp, step, R):
    h, w = tmpl.shape
    cx, cy = centre(h, w)
    x, y = sample_grid(h, w, step)
    u, v, den, xn, yn, xp, yp = warp_h(hp, x, y, cx, cy, R)
    ok = den > 1e-3
    u, v = np.where(ok, u, np.nan), np.where(ok, v, np.nan)
    valid, iw, gx, gy = sample(img, u, v)
    ir = tmpl[y[valid].astype(np.int64), x[valid].astype(np.int64)]
    return iw, ir, jac_h(gx, gy, xn[valid], yn[valid], xp[valid], yp[valid], den[valid], R)


# --------------------------------------------------------------------------------------------------------- the solver
class Result:
    """M (2 x 3, moving -> reference, full-resolution pixels), cc, iters, failed; M9 / cc / iters of the homography read-out
    when it was asked for; `steps`: one dict per step taken (level, params after it, rho at its start, status);
    `level_iters`: steps per level, coarsest first."""

    def __repr__(self):
        return "Result(cc=%r, iters=%r, failed=%r, level_iters=%r)" % (self.cc, self.iters, self.failed, self.level_iters)


def _sim_matrix(a, b, T):
    return np.array([[a, -b, T[0]], [b, a, T[1]], [0.0, 0.0, 1.0]])


def solve_pyramids(tmpl_lv, img_lv, s=1, max_iters=60, eps=1e-9, M_init=None, levels=None, homography=False,
                   min_samples=MIN_SAMPLES):
    """The estimate of the frame whose pyramid is `img_lv` against the template pyramid `tmpl_lv` (finest first)."""
    if max_iters < 1:
        max_iters = 50
    if not eps > 0:
        eps = 1e-8
    nl = len(tmpl_lv)
    a, b, T = 1.0, 0.0, np.zeros(2)
    l_first = nl - 1
    if M_init is not None:
        l_first = min(max((levels or 1) - 1, 0), nl - 1)
        Mi = np.asarray(M_init, np.float64).reshape(2, 3)
        A = np.linalg.inv(np.array([[Mi[0, 0], -Mi[1, 0]], [Mi[1, 0], Mi[0, 0]]]))
        a, b = A[0, 0], A[1, 0]
        T = -(A @ Mi[:, 2]) / (s * 2.0 ** l_first)
    r = Result()
    r.steps, r.level_iters = [], []
    failed, rho, iters = False, -1.0, 0
    t = np.zeros(2)
    for lvl in range(l_first, -1, -1):
        tm, im = tmpl_lv[lvl], img_lv[lvl]
        h, w = tm.shape
        c = np.array(centre(h, w))
        reach = math.hypot(c[0], c[1])
        step = sample_step(h * w, min_samples)
        A = np.array([[a, -b], [b, a]])
        t = T - c + A @ c
        last_rho, k = -2.0, 0
        while not failed and k < max_iters:
            k += 1
            iters += 1
            status, rho_k, dp = ecc_step(*sim_terms(tm, im, (a, b, t[0], t[1]), step))
            if status == "fail":
                failed = True
                r.steps.append(dict(level=lvl, params=(a, b, t[0], t[1]), rho=rho, status=status))
                break
            rho = rho_k
            if status == "stop":
                r.steps.append(dict(level=lvl, params=(a, b, t[0], t[1]), rho=rho, status=status))
                break
            a, b, t = a + dp[0], b + dp[1], t + dp[2:]
            r.steps.append(dict(level=lvl, params=(a, b, t[0], t[1]), rho=rho, status=status))
            move = (abs(dp[0]) + abs(dp[1])) * reach + abs(dp[2]) + abs(dp[3])
            stop = move < STOP_MOVE or abs(rho - last_rho) < eps
            last_rho = rho
            if stop:
                break
        r.level_iters.append(k)
        A = np.array([[a, -b], [b, a]])
        T = t + c - A @ c
        if lvl > 0:
            T = 2.0 * T
    bad = failed or not (a * a + b * b > 1e-12)
    if bad:
        M = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    else:
        M = np.linalg.inv(_sim_matrix(a, b, T))[:2]
        M[:, 2] *= s
    r.M, r.cc, r.iters, r.failed = M, (-2.0 if bad else rho), iters, bad
    r.params = (a, b, t[0], t[1])
    if homography:
        _homography(r, tmpl_lv[0], img_lv[0], s, max_iters, eps, t, min_samples)
    return r


def _homography(r, tm, im, s, max_iters, eps, t, min_samples):
    h, w = tm.shape
    cx, cy = centre(h, w)
    R = norm_radius(h, w)
    a, b = r.params[0], r.params[1]
    hp = np.array([a, -b, t[0] / R, b, a, t[1] / R, 0.0, 0.0])
    rho, last_rho, k, gfail = r.cc if not r.failed else -2.0, -2.0, 0, r.failed
    step = sample_step(h * w, min_samples)
    r.h_steps = []
    while not gfail and k < max_iters:
        k += 1
        status, rho_k, dp = ecc_step(*h_terms(tm, im, hp, step, R))
        if status == "fail":
            gfail = True
            break
        rho = rho_k
        if status == "stop":
            break
        hp = hp + dp
        r.h_steps.append(dict(params=hp.copy(), rho=rho))
        stop = np.abs(dp).sum() * R < STOP_MOVE or abs(rho - last_rho) < eps
        last_rho = rho
        if stop:
            break
    r.h_params, r.h_rho, r.h_iters, r.h_failed = hp, rho, k, gfail
    r.h_used = not r.failed and not gfail and k > 0 and rho >= r.cc - 1e-9
    M9 = np.vstack([r.M, [0.0, 0.0, 1.0]])
    cc9, it9 = r.cc, r.iters
    if r.h_used:
        Hn = np.append(hp, 1.0).reshape(3, 3)
        left = np.array([[s * R, 0, s * cx], [0, s * R, s * cy], [0, 0, 1.0]])      # S(s) T(c) S(R)
        right = np.array([[1 / (s * R), 0, -cx / R], [0, 1 / (s * R), -cy / R], [0, 0, 1.0]])
        W = left @ Hn @ right
        Mi = np.linalg.inv(W)
        M9 = Mi / Mi[2, 2]
        cc9, it9 = rho, r.iters + k
    r.M9, r.cc9, r.iters9 = M9, cc9, it9


def estimate(ref, mov, s=1, area=False, max_levels=0, **kw):
    """The estimate of `mov` against `ref` (H x W x 3 u8 / u16); keyword arguments as solve_pyramids."""
    return solve_pyramids(frame_pyramid(ref, s, area, max_levels), frame_pyramid(mov, s, area, max_levels), s=s, **kw)


def corner_deviation(M1, M2, h, w):
    """Largest distance between where two transforms (2 x 3 or 3 x 3) put the four corners of an h x w frame."""
    def full(M):
        M = np.asarray(M, np.float64)
        return np.vstack([M, [0.0, 0.0, 1.0]]) if M.shape == (2, 3) else M
    pts = np.array([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1]], np.float64).T
    p, q = full(M1) @ pts, full(M2) @ pts
    return float(np.hypot(*(p[:2] / p[2] - q[:2] / q[2])).max())
