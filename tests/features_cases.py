"""Scenes and cases for the feature estimator's tests (tests/features_restatement.py is the specification).

A scene is a canvas of random overlapping rectangles; the reference frame is a crop of it and the moving frame samples the
canvas bilinearly through a known transform, so `M_true` maps the moving frame onto the reference frame exactly.  Both frames
get independent Gaussian noise of 1.5 grey levels.  Everything is generated from seeds: no files.
"""
import numpy as np

import features_restatement as fr

MARGIN = 48


def canvas(h, w, seed, n_rect=None):
    """(h + 2 MARGIN) x (w + 2 MARGIN) x 3 float64 of random rectangles"""
    rng = np.random.default_rng(seed)
    hh, ww = h + 2 * MARGIN, w + 2 * MARGIN
    c = np.full((hh, ww, 3), 90.0)
    for _ in range(n_rect or (h * w) // 500):
        rh, rw = rng.integers(8, 56, 2)
        y, x = rng.integers(-8, hh - 8), rng.integers(-8, ww - 8)
        c[max(y, 0):y + rh, max(x, 0):x + rw] = rng.integers(20, 236, 3).astype(np.float64)
    return c


def sample(c, xs, ys):
    """bilinear samples of the canvas at canvas positions (xs, ys), all inside"""
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    fx, fy = (xs - x0)[..., None], (ys - y0)[..., None]
    return (c[y0, x0] * (1 - fx) * (1 - fy) + c[y0, x0 + 1] * fx * (1 - fy) + c[y0 + 1, x0] * (1 - fx) * fy
            + c[y0 + 1, x0 + 1] * fx * fy)


def blur(img, sigma):
    r = int(np.ceil(3 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    p = np.pad(img, ((r, r), (r, r), (0, 0)), mode="edge")
    p = sum(k[i] * p[i:i + img.shape[0]] for i in range(2 * r + 1))
    return sum(k[i] * p[:, i:i + img.shape[1]] for i in range(2 * r + 1))


def similarity(angle_deg, scale, tx, ty, h, w):
    """3 x 3: rotation and scale about the frame's centre, then a shift"""
    a = np.deg2rad(angle_deg)
    c, s = scale * np.cos(a), scale * np.sin(a)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0.0, 0.0, 1.0]])


def pair(h, w, m_true, seed, sigma=0.0, noise=1.5, dtype=np.uint8):
    """(moving, reference) BGR frames with reference(M_true p) = moving(p)"""
    c = canvas(h, w, seed)
    rng = np.random.default_rng(seed + 1000)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    den = m_true[2, 0] * xs + m_true[2, 1] * ys + m_true[2, 2]
    u = (m_true[0, 0] * xs + m_true[0, 1] * ys + m_true[0, 2]) / den
    v = (m_true[1, 0] * xs + m_true[1, 1] * ys + m_true[1, 2]) / den
    assert u.min() > -MARGIN + 1 and v.min() > -MARGIN + 1 and u.max() < w + MARGIN - 2 and v.max() < h + MARGIN - 2
    mov = sample(c, u + MARGIN, v + MARGIN)
    ref = c[MARGIN:MARGIN + h, MARGIN:MARGIN + w].copy()
    if sigma > 0:
        mov = blur(mov, sigma)
    out = []
    for f in (mov, ref):
        f = np.clip(np.rint(f + rng.normal(0.0, noise, f.shape)), 0, 255).astype(np.uint8)
        out.append(f if dtype == np.uint8 else (f.astype(np.uint16) << 8) | 0x5A)
    return out[0], out[1]


def corner_error(m, m_true, h, w):
    """the largest distance between the images of the four frame corners under `m` (2 x 3 or 3 x 3) and under `m_true`"""
    m = np.vstack([m, [0.0, 0.0, 1.0]]) if np.asarray(m).shape == (2, 3) else np.asarray(m)
    pts = np.array([[0.0, 0.0, 1.0], [w - 1.0, 0.0, 1.0], [0.0, h - 1.0, 1.0], [w - 1.0, h - 1.0, 1.0]]).T
    a, b = m @ pts, m_true @ pts
    return float(np.sqrt(((a[:2] / a[2] - b[:2] / b[2]) ** 2).sum(axis=0)).max())


def scene_similarity():
    h, w = 240, 320
    m = similarity(2.0, 1.02, 5.3, -3.7, h, w)
    return (h, w, m) + pair(h, w, m, 11)


def scene_homography():
    h, w = 240, 320
    m = similarity(-1.5, 0.99, -4.2, 2.6, h, w)
    m[2, 0], m[2, 1] = 4e-5, -3e-5
    return (h, w, m) + pair(h, w, m, 12)


def scene_defocus():
    h, w = 480, 640
    m = similarity(1.0, 1.015, 3.4, 2.2, h, w)
    return (h, w, m) + pair(h, w, m, 13, sigma=2.0)


# ---- frames for the stage tests
def checkerboard(h, w, cell=4, lo=40, hi=200):
    """a checkerboard of cell x cell fields whose bright fields hold a 2 x 2 bright core only (a full checkerboard has nothing
    but X junctions, which FAST does not score): the four pixels of every core score alike, so the suppression meets a tie
    at every corner"""
    y, x = np.mgrid[0:h, 0:w]
    field = ((y // cell) + (x // cell)) % 2 == 0
    return np.where(field & (y % cell < 2) & (x % cell < 2), hi, lo).astype(np.uint8)


def random_gray(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def dots(h, w, step=12, value=255, base=30):
    """a periodic frame of isolated bright pixels: every dot scores the same"""
    g = np.full((h, w), base, np.uint8)
    g[EDGE_OFF::step, EDGE_OFF::step] = value
    return g


EDGE_OFF = 18


def score_shapes(tile_h, tile_w):
    """one scoring pixel, none, and one row / column short of, on, and one past the score kernel's tile grid"""
    out = [(33, 33), (32, 40)]
    for dh in (-1, 0, 1):
        out.append((3 * tile_h + dh, 2 * tile_w + dh))
    return out


# ---- RANSAC cases: (name, kind, n, k, seed).  Points: a known model on random positions in a 64 x 64 square, 60 % inliers
# with 0.3 px noise, the rest uniformly wrong.  The square is small on purpose: the unnormalised 8 x 8 system of a homography
# has entries 1 and u * x side by side, and the GPU test's model tolerance (eps times the condition number) wants that
# number capped -- samples whose system is conditioned worse than COND_KEEP are not put into the table.
RANSAC_CASES = [(f"{'sim' if kind == fr.SIMILARITY else 'hom'}_n{n}_k{k}", kind, n, k, 7 * n + k + kind)
                for kind in (fr.SIMILARITY, fr.HOMOGRAPHY)
                for n, k in ((2, 1), (4, 1), (4, 64), (63, 64), (64, 64), (65, 64), (1000, 64), (1000, 2000), (64, 2000))
                if n >= (4 if kind == fr.HOMOGRAPHY else 2)]
RANSAC_THR = 3.0
SIDE = 64.0
COND_CAP, COND_KEEP = 1e6, 5e5


def ransac_points(kind, n, seed):
    rng = np.random.default_rng(seed)
    src = rng.uniform(0.0, SIDE, (n, 2))
    m = similarity(3.0, 1.03, 6.0, -4.0, SIDE, SIDE)
    if kind == fr.HOMOGRAPHY:
        m[2, 0], m[2, 1] = 3e-4, -2e-4
    p = np.concatenate([src, np.ones((n, 1))], axis=1) @ m.T
    dst = p[:, :2] / p[:, 2:] + rng.normal(0.0, 0.3, (n, 2))
    bad = rng.random(n) > 0.6
    if n > 8:
        dst[bad] = rng.uniform(0.0, SIDE, (int(bad.sum()), 2))
    return src, dst


def system_conds(src, dst, samples):
    """the 2-norm condition number of every sample's 8 x 8 homography system"""
    return np.array([np.linalg.cond(fr.homography_system(src, dst, s)[:, :8]) for s in samples])


def ransac_case(kind, n, k, seed):
    src, dst = ransac_points(kind, n, seed)
    if kind == fr.SIMILARITY:
        return src, dst, fr.sample_table(n, k, 2, seed)
    cand = fr.sample_table(n, 4 * k + 32, 4, seed)
    keep = cand[system_conds(src, dst, cand) <= COND_KEEP]
    assert len(keep) > 0, "no well-conditioned sample"
    return src, dst, np.ascontiguousarray(np.resize(keep, (k, 4)))


def degenerate_case(kind):
    """samples with coincident (similarity) and collinear or repeated (homography) points beside one good one"""
    src, dst = ransac_points(kind, 16, 99)
    src, dst = src.copy(), dst.copy()
    if kind == fr.SIMILARITY:
        src[1] = src[0]
        return src, dst, np.array([[0, 1], [2, 3], [1, 0]], np.int32)
    src[0:4] = [[10.0, 5.0], [20.0, 5.0], [30.0, 5.0], [45.0, 5.0]]      # four collinear source points
    src[5], dst[5] = src[4], dst[4]                  # and a coincident pair
    return src, dst, np.array([[0, 1, 2, 3], [8, 9, 10, 11], [4, 5, 6, 7]], np.int32)


# ---- extraction cases: name -> (frame, levels, n_features, threshold, what the restatement must find: "some", "none",
# "short" (corners exist but level 0 keeps fewer than n_features: one score class overflows the capacity), "two_levels")
def extract_cases():
    _, _, _, _, ref = scene_similarity()
    g = fr.gray(ref)
    u16 = (ref.astype(np.uint16) << 8) | 0x3C
    return {
        "bgr_u8_l3": (ref, 3, 2000, 20, "some"),
        "bgr_u16_l3": (u16, 3, 2000, 20, "some"),
        "gray_u8_l1": (g, 1, 2000, 20, "some"),
        "gray_u16_l3": ((g.astype(np.uint16) << 8) | 0xC3, 3, 100, 20, "some"),
        "dots_n8": (dots(240, 320), 1, 8, 20, "some"),
        "dots_overflow": (dots(300, 400, step=4), 1, 8, 20, "short"),
        "small_for_level2": (ref[:100, :100], 3, 2000, 20, "two_levels"),
        "flat": (np.full((120, 160, 3), 77, np.uint8), 3, 2000, 20, "none"),
    }
