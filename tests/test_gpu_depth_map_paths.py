"""GPU: every DepthMapStack kernel path (csrc/kernels_depthmap.hpp, dispatch in csrc/depthmap_host.hpp) against
oracle/depth_map_oracle.py, stage by stage.  tests/test_gpu_depth_map.py compares final images at mostly single-tile
sizes; TABLE below names, row by row, the kernel instantiation and the branch a case is there for, at sizes worked out
from the kernels' own tile constants, and the handle's taps (mi_dmap_tap) carry the comparison into the float planes.

What a case asserts, in the order that makes a failure name its stage:
  1. raw energies (tap, after push): np.array_equal -- -ffp-contract=off, the oracle's operation order, no transcendental.
  2. the focus map's input per frame, the total and (MAX map) the maximum plane (taps, after finish):
     no smoothing and AVERAGE map -> np.array_equal (divisions only).  Otherwise an exp is behind the plane (the bilateral
     range table, the softmax) and the only admissible deviation is what one last bit of that exp can do: the oracle's
     stage is run again with every exp moved one value up and one down (exp_ulp=+1 / -1), the bound per plane kind is
     2 x the larger spread (the factor for accumulation the two probes do not span).  The MI355X run showed every such
     plane BIT-EQUAL except the rows tagged in EXP_BOUND, so equality is what is asserted for all others and the derived
     bound only for those; the probes are computed only when a plane is not bit-equal.  Measured spreads: SPREADS below.
  3. the final image: the project's rule (<= 1 count on <= 0.1 % of the values: a cap, not a measurement), bit-equality
     for every row without smoothing on the AVERAGE map, and the number of bit-equal images over the table.
"""
import numpy as np
import pytest

from oracle import depth_map_oracle as dmo
from test_gpu_depth_map import ENERGY, MAP, close_enough, scene

pytestmark = pytest.mark.gpu

# ---- tile arithmetic, from the kernel file's constants
TW = 64                      # every dm_* tile is 64 wide
LAP5_TH = 32                 # dm_energy_lap5: TH; interior when x0 >= 4, y0 >= 4, x0 + TW + 4 <= w, y0 + TH + 4 <= h
LAP5_W, LAP5_H = TW + TW + 4, LAP5_TH + LAP5_TH + 4          # 132, 68: smallest frame with an interior tile (tile 1, 1)
PD_W = 2 * TW - 2 + (2 * (TW - 1) + 5) + 2                   # 259: dm_pyrdown_tile interior at x0 = 64 (IW + 2 padding bytes' worth)


def pd_h(th):                # 4 TH + 1: interior at y0 = TH (2 y0 - 2 + IH <= h, IH = 2 (TH - 1) + 5)
    return 4 * th + 1


PD_TH = {("u8", 3, "f"): 16, ("u16", 3, "f"): 16, ("f", 3, "f"): 8, ("f", 1, "f"): 16, ("d", 1, "d"): 8}   # dm_pyrdown_tile_rows
BIL_ROWS, LAP_ROWS = 4 * 6, 4 * 4    # 4 * DM_BIL_NP rows per dm_bilateral tile, 4 * DM_LAP_ROWS per dm_laplacian_rows tile
DM_FMM_FRAMES = 4096
assert (LAP5_W, LAP5_H, PD_W, pd_h(16), pd_h(8)) == (132, 68, 259, 65, 33)

u8, u16 = np.uint8, np.uint16
F64 = {"float_type": "float-64"}

# (tag, dtype, n, h, w, kwargs, generator).  Default kwargs: laplacian 5 / blur 5 / smooth 15 / average / levels 3 / float-32.
TABLE = [
    # ---- float-64, >= 3 tiles each way (dm_blur / dm_sobel tiles are 4 x 64, dm_laplacian_rows 16 x 64, dm_bilateral 24 x 64,
    # dm_lap_blend_quad 8 x 128), 530 wide so that level 1 (265 wide) still has an interior dm_pyrdown_tile column
    # dm_gray<u16,double>, dm_blur<.,double>, dm_laplacian_rows<5,double>, dm_normalise<double>, dm_to_f32, dm_bilateral<6,7>,
    # dm_pyrdown<u16,3,double>, dm_pyrdown<double,3,double>, dm_pyrdown_tile<float,1,float,16> (interior: 70 >= 65),
    # dm_lap_blend_quad<u16,double,float>, dm_top_blend<double,double,float>, dm_collapse_quad<double>, dm_finalize<u16,double>
    ("f64-lap5-smooth-avg-u16", u16, 2, 70, 530, {**F64}, "scene"),
    # dm_pyrdown_tile<double,1,double,8> interior at level 0 -> 1 (530 >= 259, 70 >= 33) and 1 -> 2 (265 >= 259, 35 >= 33),
    # dm_accumulate<double>, dm_weight<double>, dm_lap_blend_quad<u16,double,double>
    ("f64-lap5-nosmooth-avg-u16", u16, 3, 70, 530, {**F64, "smooth_size": 0}, "scene"),
    # dm_laplacian_rows<3,double>, dm_relative<double> (MAX map, exp in double), dm_accumulate<double> mode max, u8 frames
    ("f64-lap3-nosmooth-max-u8", u8, 2, 70, 530, {**F64, "kernel_size": 3, "smooth_size": 0, "map_type": "max"}, "scene"),
    # dm_laplacian<0,double> aperture 9, blur 11 (computed taps), dm_bilateral<6,0> radius 2, MAX map on float32 weights
    ("f64-lap9-smooth5-max-u8", u8, 2, 70, 530, {**F64, "kernel_size": 9, "blur_size": 11, "smooth_size": 5, "map_type": "max",
                                                  "levels": 4}, "scene"),
    # dm_sobel<double>, no smoothing, AVERAGE
    ("f64-sobel-nosmooth-avg-u16", u16, 2, 70, 530, {**F64, "energy": "sobel", "smooth_size": 0}, "blocks"),
    # dm_sobel<double> with smoothing (default radius), MAX map
    ("f64-sobel-smooth-max-u8", u8, 2, 70, 530, {**F64, "energy": "sobel", "map_type": "max", "temperature": 0.05}, "scene"),

    # ---- float-32 dm_pyrdown_tile, interior and rim of every instantiation; the interior test holds with EQUALITY at
    # source width 259 (x0 = 64) and source height 4 TH + 1, and fails one below
    # <uint8_t,3,float,16> and <float,1,float,16> at level 0 -> 1: 65 x 259 is exactly interior ...
    ("pd-u8-interior-eq", u8, 2, 65, 259, {"levels": 2, "smooth_size": 5}, "scene"),
    # ... 258 wide is not (rim path everywhere), nor is 64 high
    ("pd-u8-rim-w258", u8, 2, 65, 258, {"levels": 2, "smooth_size": 5}, "scene"),
    ("pd-u8-rim-h64", u8, 2, 64, 259, {"levels": 2, "smooth_size": 5}, "scene"),
    # <uint16_t,3,float,16>: the same three
    ("pd-u16-interior-eq", u16, 2, 65, 259, {"levels": 2, "smooth_size": 0}, "scene"),
    ("pd-u16-rim-w258", u16, 2, 65, 258, {"levels": 2, "smooth_size": 0}, "scene"),
    ("pd-u16-interior-2x2", u16, 2, 100, 400, {"levels": 2}, "blocks"),          # tiles (1..2, 1..2) interior, the rest rim
    # <float,3,float,8> at level 1 -> 2: level 1 of 65 x 517 is 33 x 259, exactly interior (TH = 8: 33 rows); 516 -> 258 is not
    ("pd-f3-interior-eq", u16, 2, 65, 517, {"levels": 3, "smooth_size": 5}, "scene"),
    ("pd-f3-rim-w516", u16, 2, 65, 516, {"levels": 3, "smooth_size": 5}, "scene"),
    ("pd-f3-rim-h64", u8, 2, 64, 517, {"levels": 3, "smooth_size": 0}, "scene"),
    # <float,1,float,16> at level 1 -> 2 (the weight pyramid): level 1 must be 65 x 259 -> frame 129 x 517
    ("pd-f1-level1-interior-eq", u16, 2, 129, 517, {"levels": 3, "smooth_size": 3}, "scene"),
    # levels 4 on 261 x 1034: level 2 is 66 x 259, so level 2 -> 3 has interior tiles in <float,3,float,8> and <float,1,float,16>
    ("pd-level2-interior", u16, 2, 261, 1034, {"levels": 4, "smooth_size": 5}, "scene"),
    ("pd-level2-interior-max-u8", u8, 2, 261, 1034, {"levels": 5, "smooth_size": 0, "map_type": "max"}, "blocks"),
]
# ---- dm_energy_lap5<uint8_t> / <uint16_t>, folded (smooth_size > 0: per-frame min / max through fmm, dm_bilateral divides as
# it stages) and unfolded (smooth_size 0: dm_normalise<float>): one below, at and one above the interior thresholds
# (w 131 / 132 / 133, h 67 / 68 / 69), a last tile 1, 3 and 63 columns wide (129, 131, 191), the smallest frame that takes
# this kernel (8 x 8) and one that does not (h = 7: dm_gray / dm_blur / dm_laplacian_rows<5,float>)
for _dt in (u8, u16):
    for _sm in (15, 0):
        for _h, _w in ((67, 131), (68, 132), (69, 133), (68, 131), (67, 132), (40, 129), (33, 191), (8, 8), (7, 8), (9, 65)):
            TABLE.append((f"lap5-{np.dtype(_dt).name}-{'folded' if _sm else 'unfolded'}-{_h}x{_w}", _dt, 3, _h, _w,
                          {"smooth_size": _sm}, "scene" if (_h + _w) % 2 else "blocks"))
TABLE += [
    # ---- the separate energy kernels over 5 x 3 (dm_laplacian_rows) / 18 x 3 (dm_laplacian, dm_sobel, dm_blur) tiles, float-32
    # dm_laplacian_rows<3,float>, blur 3
    ("sep-lap3", u16, 2, 70, 150, {"kernel_size": 3, "blur_size": 3, "smooth_size": 0}, "scene"),
    # dm_laplacian<0,float>: aperture 1 (the fixed 3 x 3 cross) with blur 1, 7 with blur 7, 15 with blur 31 (computed taps)
    ("sep-lap1-blur1", u16, 2, 70, 150, {"kernel_size": 1, "blur_size": 1, "smooth_size": 0}, "scene"),
    ("sep-lap7-blur7", u16, 2, 70, 150, {"kernel_size": 7, "blur_size": 7, "smooth_size": 0, "map_type": "max"}, "scene"),
    ("sep-lap15-blur31", u16, 2, 70, 150, {"kernel_size": 15, "blur_size": 31, "smooth_size": 0}, "blocks"),
    # blur sizes on the default aperture: dm_laplacian_rows<5,float> after dm_blur with 31 taps (unfolded smoothing path:
    # dm_normalise<float> feeds the bilateral filter its min / max)
    ("sep-lap5-blur31-smooth", u16, 2, 70, 150, {"blur_size": 31}, "scene"),
    # dm_sobel<float>, with and without smoothing
    ("sep-sobel", u16, 3, 70, 150, {"energy": "sobel", "smooth_size": 0}, "blocks"),
    ("sep-sobel-smooth", u8, 3, 70, 150, {"energy": "sobel"}, "scene"),
    # ---- dm_bilateral over 3 x 3 tiles (24 x 64): radius 7 (<6,7>), radius 1 and radius 15 (<6,0>), and frames narrower /
    # lower than the radius, where every tap reflects (more than once at 5 wide)
    ("bil-r7", u16, 2, 70, 150, {}, "scene"),
    ("bil-r1", u16, 2, 70, 150, {"smooth_size": 3}, "scene"),
    ("bil-r15", u16, 2, 70, 150, {"smooth_size": 31}, "scene"),
    ("bil-r15-narrow", u16, 2, 70, 5, {"smooth_size": 31}, "scene"),
    ("bil-r15-low", u16, 2, 11, 150, {"smooth_size": 31, "map_type": "max"}, "scene"),
    ("bil-r7-narrow-lap5", u8, 2, 50, 9, {}, "blocks"),
    # ---- above 1 048 576 pixels, both sides odd (dm_normalise's grid is capped at 4096 blocks there; n % 4 = 3: its scalar tail)
    ("mp1-sobel-unfolded", u16, 2, 1031, 1045, {"energy": "sobel", "smooth_size": 0}, "scene"),
    ("mp1-default-folded", u16, 2, 1031, 1045, {}, "scene"),
    # dm_normalise reads four values per thread, so its grid-stride loop takes a SECOND step only above 4 x 1 048 576 pixels
    ("mp4-sobel-unfolded-gridstride", u16, 2, 2049, 2051, {"energy": "sobel", "smooth_size": 0, "levels": 2}, "scene"),
    # ---- more frames than fmm slots: frames 0 .. 4095 folded, 4096 .. 4099 through dm_normalise<float>, in one stack
    ("fmm-4100-frames", u8, DM_FMM_FRAMES + 4, 8, 9, {}, "many"),
    # ---- frames that stress the normalisation (multi-tile, default = folded path)
    ("norm-flat-frame", u16, 3, 70, 150, {}, "flatframe"),              # one frame with zero energy everywhere (flat: lut skipped)
    ("norm-flat-frame-max", u16, 3, 70, 150, {"map_type": "max"}, "flatframe"),
    ("norm-flat-band", u16, 3, 70, 150, {}, "flatband"),                # zero total in a band: weights 0 (see the test below)
    ("norm-flat-band-nosmooth", u16, 3, 70, 150, {"smooth_size": 0}, "flatband"),
    ("norm-max-in-last-tile", u16, 3, 70, 150, {}, "maxlast"),          # the global maximum in the last frame's last tile
    ("norm-max-in-last-tile-unfolded", u16, 3, 70, 150, {"smooth_size": 0}, "maxlast"),
    ("norm-u16-full-range", u16, 3, 70, 150, {}, "blocks"),             # 0 and 65535 side by side
    ("norm-u16-full-range-f64", u16, 3, 70, 150, {**F64, "smooth_size": 0}, "blocks"),
]
TAGS = [r[0] for r in TABLE]
assert len(set(TAGS)) == len(TAGS)

# Rows whose exp-dependent planes are NOT bit-equal on the MI355X and are held to the derived bound instead (all others:
# equality).  The one row is the float-64 softmax: dm_relative<double> calls the device library's exp, the oracle's is the
# correctly rounded one; measured deviation 1.1e-16 (energy_in) / 2.2e-16 (tot) against bounds of 4.4e-16 / 8.9e-16.
# Every plane behind the float32 range table or the float32 softmax (exp in double, rounded once) was bit-equal.
EXP_BOUND = {"f64-lap3-nosmooth-max-u8"}
# bit-equal final images the MI355X run showed over the whole table (a regression from identical to within-tolerance shows here)
EXACT_IMAGES = 83

# Measured on the CPU (oracle alone): largest |plane(exp_ulp = +-1) - plane(0)| per plane kind, the bound being twice that.
SPREADS = """
f64-lap5-smooth-avg-u16: energy_in=1.19e-07 tot=1.79e-07
f64-lap3-nosmooth-max-u8: energy_in=2.22e-16 tot=4.44e-16 mx=0
f64-lap9-smooth5-max-u8: energy_in=1.55e-06 tot=1.67e-06 mx=1.49e-07
f64-sobel-smooth-max-u8: energy_in=2.15e-06 tot=2.26e-06 mx=1.49e-07
pd-u8-interior-eq: energy_in=1.19e-07 tot=1.79e-07
pd-u8-rim-w258: energy_in=1.19e-07 tot=2.38e-07
pd-u8-rim-h64: energy_in=1.19e-07 tot=1.79e-07
pd-u16-interior-2x2: energy_in=1.19e-07 tot=1.79e-07
pd-f3-interior-eq: energy_in=1.19e-07 tot=1.79e-07
pd-f3-rim-w516: energy_in=1.19e-07 tot=1.19e-07
pd-f1-level1-interior-eq: energy_in=1.49e-07 tot=2.38e-07
pd-level2-interior: energy_in=1.19e-07 tot=1.79e-07
pd-level2-interior-max-u8: energy_in=1.19e-07 tot=2.38e-07 mx=0
lap5-uint8-folded-67x131: energy_in=1.19e-07 tot=2.38e-07
lap5-uint8-folded-68x132: energy_in=1.49e-07 tot=2.38e-07
lap5-uint8-folded-69x133: energy_in=1.19e-07 tot=2.38e-07
lap5-uint8-folded-68x131: energy_in=8.94e-08 tot=2.38e-07
lap5-uint8-folded-67x132: energy_in=1.19e-07 tot=2.38e-07
lap5-uint8-folded-40x129: energy_in=1.19e-07 tot=2.38e-07
lap5-uint8-folded-33x191: energy_in=1.19e-07 tot=1.79e-07
lap5-uint8-folded-8x8: energy_in=7.45e-08 tot=1.19e-07
lap5-uint8-folded-7x8: energy_in=1.19e-07 tot=2.38e-07
lap5-uint8-folded-9x65: energy_in=8.94e-08 tot=1.79e-07
lap5-uint16-folded-67x131: energy_in=1.19e-07 tot=2.38e-07
lap5-uint16-folded-68x132: energy_in=8.94e-08 tot=1.79e-07
lap5-uint16-folded-69x133: energy_in=1.19e-07 tot=2.38e-07
lap5-uint16-folded-68x131: energy_in=1.04e-07 tot=2.38e-07
lap5-uint16-folded-67x132: energy_in=1.04e-07 tot=1.79e-07
lap5-uint16-folded-40x129: energy_in=1.04e-07 tot=2.38e-07
lap5-uint16-folded-33x191: energy_in=1.49e-07 tot=2.38e-07
lap5-uint16-folded-8x8: energy_in=7.45e-08 tot=1.19e-07
lap5-uint16-folded-7x8: energy_in=8.94e-08 tot=2.38e-07
lap5-uint16-folded-9x65: energy_in=1.19e-07 tot=2.38e-07
sep-lap7-blur7: energy_in=1.19e-07 tot=2.38e-07 mx=0
sep-lap5-blur31-smooth: energy_in=1.79e-07 tot=2.38e-07
sep-sobel-smooth: energy_in=1.19e-07 tot=2.38e-07
bil-r7: energy_in=8.94e-08 tot=1.19e-07
bil-r1: energy_in=1.79e-07 tot=2.38e-07
bil-r15: energy_in=1.04e-07 tot=1.49e-07
bil-r15-narrow: energy_in=8.94e-08 tot=1.19e-07
bil-r15-low: energy_in=8.34e-07 tot=9.54e-07 mx=8.94e-08
bil-r7-narrow-lap5: energy_in=8.94e-08 tot=8.94e-08
mp1-default-folded: energy_in=1.04e-07 tot=1.19e-07
norm-flat-frame: energy_in=1.19e-07 tot=2.38e-07
norm-flat-frame-max: energy_in=1.49e-07 tot=4.77e-07 mx=8.94e-08
norm-flat-band: energy_in=8.94e-08 tot=2.38e-07
norm-max-in-last-tile: energy_in=5.96e-08 tot=5.96e-08
norm-u16-full-range: energy_in=1.04e-07 tot=1.79e-07
fmm-4100-frames: not probed (two more 40 s oracle runs; its planes are bit-equal)
"""


def blocks(rng, n, h, w, dtype):
    """Hard edges and saturated areas: rectangles of constant colour (0 and full scale among them) on a constant ground;
    frame i keeps them sharp in one part and box-blurred elsewhere.  Energies have exact zeros and exact ties."""
    top = 255 if dtype == np.uint8 else 65535
    base = np.full((h, w, 3), top // 3, np.float64)
    for _ in range(min(max(4, h * w // 400), 300)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        hh, ww = int(rng.integers(1, max(2, h // 3))), int(rng.integers(1, max(2, w // 3)))
        base[y:y + hh, x:x + ww] = rng.choice([0, top, top, 0, int(rng.integers(0, top + 1))], 3)
    soft = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4
    out = []
    for i in range(n):
        f = soft.copy()
        lo, hi = (w * i) // n, (w * (i + 1)) // n
        f[:, lo:hi] = base[:, lo:hi]
        out.append(np.floor(f).astype(dtype))
    return out


def make_frames(tag, dtype, n, h, w, gen):
    rng = np.random.default_rng(500 + TAGS.index(tag))
    if gen == "blocks":
        return blocks(rng, n, h, w, dtype)
    top = 255 if dtype == np.uint8 else 65535
    if gen == "many":   # thousands of tiny frames: one texture at a contrast and under a noise that change from frame to frame
        base = rng.random((h, w, 3))
        return [((base * ((i % 7) + 1) / 7 + rng.random((h, w, 3)) * 0.2 * (i % 5)) * (top / 1.8)).astype(dtype) for i in range(n)]
    frames = scene(rng, n, h, w, dtype)
    if gen == "flatframe":
        frames[1][:] = top // 5
    elif gen == "flatband":
        for f in frames:
            f[:, 40:100] = top // 2            # 60 columns: wider than blur + aperture + bilateral disc on both sides
    elif gen == "maxlast":
        for f in frames:
            f //= 4                            # low contrast everywhere ...
        frames[-1][h - 6:, w - 6:] = 0
        frames[-1][h - 4:h - 1, w - 4:w - 1] = top   # ... but for a full-scale spot on black in the last corner
    return frames


def gpu_stages(L, frames, dm=None, **kw):
    """push / tap / finish / tap on a handle (a fresh one unless given): the oracle's stages as the GPU holds them"""
    kw = dict(kw)
    h, w = frames[0].shape[:2]
    ft = L.MI_F64 if kw.pop("float_type", "float-32") == "float-64" else L.MI_F32
    mt = kw.pop("map_type", "average")
    own = dm is None
    if own:
        dm = L.DepthMap(h, w, dtype=frames[0].dtype, map_type=MAP[mt], energy=ENERGY[kw.pop("energy", "laplacian")],
                        float_type=ft, **kw)
    try:
        for f in frames:
            dm.push_frame(f)
        n = len(frames)
        assert dm.frames_pushed == n
        st = {"energy_raw": [dm.tap(L.DM_TAP_ENERGY_RAW, i) for i in range(n)]}
        st["out"] = dm.finish()
        st["energy_in"] = [dm.tap(L.DM_TAP_ENERGY_IN, i) for i in range(n)]
        st["tot"] = dm.tap(L.DM_TAP_TOTAL)
        if mt == "max":
            st["mx"] = dm.tap(L.DM_TAP_MAX)
        return st
    finally:
        if own:
            dm.close()


def same_planes(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def dev(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))))


def exp_spreads(frames, kw, want):
    """{plane kind: larger of the two spreads} from the oracle alone: its stages with every exp one value up / down"""
    probes = [dmo.depth_map_stack(frames, stages="maps", exp_ulp=u, **kw) for u in (1, -1)]
    return {k: max(dev(p[k], want[k]) for p in probes) for k in ("energy_in", "tot", "mx") if k in want}


def has_exp(kw):
    return kw.get("smooth_size", 15) > 0 or kw.get("map_type", "average") == "max"


def check_stages(tag, frames, kw, got, want):
    """rules 1-3 of the module docstring; returns whether the final image is bit-equal"""
    n = len(frames)
    for i in range(n):
        assert same_planes(got["energy_raw"][i], want["energy_raw"][i]), (tag, "raw energy", i, dev(got["energy_raw"][i], want["energy_raw"][i]))
    kinds = [k for k in ("mx", "energy_in", "tot") if k in want]
    for k in kinds:
        assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype, (tag, k)
    equal = {k: same_planes(got[k], want[k]) for k in kinds}
    devs = {k: dev(got[k], want[k]) for k in kinds}
    info = close_enough(got["out"], want["out"], what=tag)
    print(f"PATHS {tag} planes_equal={all(equal.values())} dev={devs} image={info}")
    if not all(equal.values()):
        assert has_exp(kw), (tag, "no exp behind these planes: equality is the rule", devs)
        spread = exp_spreads(frames, kw, want)
        print(f"PATHS {tag} spreads={spread}")
        for k in kinds:
            assert devs[k] <= 2 * spread[k], (tag, k, devs[k], "bound", 2 * spread[k])
        assert tag in EXP_BOUND, (tag, "planes were bit-equal on the MI355X when this table was measured", devs, spread)
    if not has_exp(kw):
        assert info[0] == 0, (tag, "no smoothing, AVERAGE map: the image is bit-equal", info)
    return info[0] == 0


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


RESULTS = {}


def run_row(L, tag):
    _, dtype, n, h, w, kw, gen = TABLE[TAGS.index(tag)]
    frames = make_frames(tag, dtype, n, h, w, gen)
    want = dmo.depth_map_stack(frames, stages=True, **kw)
    got = gpu_stages(L, frames, **kw)
    RESULTS[tag] = check_stages(tag, frames, kw, got, want)
    return frames, got, want


@pytest.mark.parametrize("tag", TAGS)
def test_path(L, tag):
    """The 4100-frame row costs about 35 s of oracle time and the three rows above 1 MP about 10 s each; the rest of
    the table is seconds."""
    frames, got, want = run_row(L, tag)
    if "flat-band" in tag:
        # zero total where every frame is flat: the reference leaves those weights uninitialised, the oracle and the GPU
        # write 0.  The weights themselves through get_focus_map's kernels (mi_dmap_planes stage 3) on the GPU's own planes
        band = np.s_[:, 60:80]
        assert np.all(want["tot"][band] == 0) and np.all(got["tot"][band] == 0)
        with L.DepthMap(*frames[0].shape[:2], dtype=frames[0].dtype, smooth_size=TABLE[TAGS.index(tag)][5].get("smooth_size", 15)) as dm:
            wg = dm.planes(3, np.stack(got["energy_in"]), np.float32)
        assert np.all(wg[(slice(None),) + band] == 0)
        assert np.array_equal(wg, np.stack(want["weights"]))
    if "max-in-last-tile" in tag:
        e = want["energy_raw"]
        h, w = e[0].shape
        y, x = np.unravel_index(np.argmax(e[-1]), e[-1].shape)
        assert e[-1].max() > max(a.max() for a in e[:-1]) and y >= h - h % LAP5_TH and x >= w - w % TW, "the row must put the maximum there"


def test_exact_image_count(L):
    """bit-identical is the rule, the image tolerance the exception: count the rule's cases over the whole table"""
    for tag in TAGS:
        if tag not in RESULTS:
            run_row(L, tag)
    exact = sum(RESULTS[t] for t in TAGS)
    print(f"PATHS exact images {exact} of {len(TAGS)}: not exact {[t for t in TAGS if not RESULTS[t]]}")
    assert exact >= EXACT_IMAGES, [t for t in TAGS if not RESULTS[t]]


def test_tap_states(L):
    """a tap outside the phase its plane exists in is refused on the host with MI_ERR_STATE (nothing is read), a frame
    that has not been pushed in this stack with MI_ERR_INVALID -- also after reset(), when the buffers still hold the
    previous stack"""
    frames = scene(np.random.default_rng(21), 2, 40, 70, u16)
    lib = L.load()
    sentinel = np.full((40, 70), -7.0, np.float32)

    def rc(dm, what, frame=0):
        out = sentinel.copy()
        r = lib.mi_dmap_tap(dm._h, what, frame, out.ctypes.data)
        if r != L.MI_OK:
            assert np.array_equal(out, sentinel), "a refused tap wrote to the caller's buffer"
        return r
    with L.DepthMap(40, 70, dtype=u16) as dm:
        assert rc(dm, L.DM_TAP_ENERGY_RAW) == L.MI_ERR_INVALID            # nothing pushed
        for what in (L.DM_TAP_ENERGY_IN, L.DM_TAP_TOTAL, L.DM_TAP_MAX):
            assert rc(dm, what) == L.MI_ERR_STATE
        dm.push_frame(frames[0])
        assert rc(dm, L.DM_TAP_ENERGY_RAW, 0) == L.MI_OK and rc(dm, L.DM_TAP_ENERGY_RAW, 1) == L.MI_ERR_INVALID
        assert rc(dm, L.DM_TAP_ENERGY_RAW, -1) == L.MI_ERR_INVALID
        assert rc(dm, L.DM_TAP_ENERGY_IN) == L.MI_ERR_STATE and rc(dm, L.DM_TAP_TOTAL) == L.MI_ERR_STATE
        dm.push_frame(frames[1])
        dm.finish()
        assert rc(dm, L.DM_TAP_ENERGY_RAW, 0) == L.MI_ERR_STATE           # normalised / smoothed in place by now
        assert b"finish" in lib.mi_last_error()
        assert rc(dm, L.DM_TAP_ENERGY_IN, 1) == L.MI_OK and rc(dm, L.DM_TAP_ENERGY_IN, 2) == L.MI_ERR_INVALID
        assert rc(dm, L.DM_TAP_TOTAL) == L.MI_OK
        assert rc(dm, L.DM_TAP_MAX) == L.MI_ERR_INVALID                   # AVERAGE map: no maximum plane
        assert rc(dm, 4) == L.MI_ERR_INVALID and rc(dm, -1) == L.MI_ERR_INVALID
        assert lib.mi_dmap_tap(dm._h, L.DM_TAP_TOTAL, 0, None) == L.MI_ERR_INVALID
        with pytest.raises(RuntimeError):
            dm.tap(L.DM_TAP_ENERGY_RAW, 0)
        dm.reset()
        # the previous stack's planes are still in the buffers: none of them may be handed out
        assert rc(dm, L.DM_TAP_ENERGY_RAW, 0) == L.MI_ERR_INVALID
        assert rc(dm, L.DM_TAP_ENERGY_IN, 0) == L.MI_ERR_STATE and rc(dm, L.DM_TAP_TOTAL) == L.MI_ERR_STATE
        dm.push_frame(frames[1])
        assert rc(dm, L.DM_TAP_ENERGY_RAW, 0) == L.MI_OK and rc(dm, L.DM_TAP_ENERGY_RAW, 1) == L.MI_ERR_INVALID
    assert lib.mi_dmap_tap(None, 0, 0, sentinel.ctypes.data) == L.MI_ERR_INVALID
    with L.DepthMap(40, 70, dtype=u16, map_type=MAP["max"]) as dm:
        dm.push_frame(frames[0])
        assert rc(dm, L.DM_TAP_MAX) == L.MI_ERR_STATE
        dm.finish()
        assert rc(dm, L.DM_TAP_MAX) == L.MI_OK


@pytest.mark.parametrize("kw", [{}, {"smooth_size": 0, "map_type": "max"}, {**F64}, {**F64, "smooth_size": 0}],
                         ids=["folded", "unfolded-max", "f64-smooth", "f64-nosmooth"])
def test_handle_reuse_across_loads(L, kw):
    """One handle, three stacks of 5, 2 and 7 frames at a multi-tile size with reset() between: what survives a reset
    (have_fmm[i], the fmm slots, the frame and energy buffers, the swapped spare plane) must not reach the next stack.
    Every stage and the image equal a fresh handle's, bit for bit."""
    rng = np.random.default_rng(33)
    h, w = 70, 150
    loads = [scene(rng, 5, h, w, u16), blocks(rng, 2, h, w, u16), scene(rng, 7, h, w, u16)]
    k = dict(kw)
    ft = L.MI_F64 if k.pop("float_type", "float-32") == "float-64" else L.MI_F32
    with L.DepthMap(h, w, dtype=u16, map_type=MAP[k.pop("map_type", "average")], float_type=ft, **k) as dm:
        for frames in loads:
            reused = gpu_stages(L, frames, dm=dm, **kw)
            dm.reset()
            fresh = gpu_stages(L, frames, **kw)
            assert np.array_equal(reused["out"], fresh["out"]), len(frames)
            for key in fresh:
                assert same_planes(reused[key], fresh[key]), (key, len(frames))
    close_enough(fresh["out"], dmo.depth_map_stack(loads[-1], **kw), what="last load")


STEP_CASES = [
    # multi-tile planes (70 x 150: 5 x 3 dm_laplacian_rows tiles, 3 x 3 dm_bilateral tiles; 133 x 260: 6 x 5 of the latter)
    ("f32-default", 70, 150, "float-32", {}),
    ("f32-lap3-blur7-r2-max", 70, 150, "float-32", {"kernel_size": 3, "blur_size": 7, "smooth_size": 5, "map_type": "max"}),
    ("f32-lap9-blur11-r15", 70, 150, "float-32", {"kernel_size": 9, "blur_size": 11, "smooth_size": 31}),
    ("f32-default-large", 133, 260, "float-32", {"map_type": "max", "temperature": 0.05}),
    ("f64-default", 70, 150, "float-64", {}),
    ("f64-lap3-blur7-r2-max", 70, 150, "float-64", {"kernel_size": 3, "blur_size": 7, "smooth_size": 5, "map_type": "max"}),
    ("f64-lap15-blur31-nosmooth-max", 70, 150, "float-64", {"kernel_size": 15, "blur_size": 31, "smooth_size": 0, "map_type": "max"}),
    ("f64-default-large-nosmooth", 133, 260, "float-64", {"smooth_size": 0}),
]
# step rows whose exp-dependent planes are not bit-equal on the MI355X (held to the derived bound); from the run
# (the float-64 softmax again: 2.2e-16 against a bound of 4.4e-16)
STEP_EXP_BOUND = {("f64-lap15-blur31-nosmooth-max", "focus map")}


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_methods_on_multi_tile_planes(L, oracle, case):
    """DepthMapStack.get_sobel_map / get_laplacian_map / smooth_energy / get_focus_map (mi_dmap_planes: the separate kernels)
    against the oracle's functions of the same stages; the rules of the module docstring: equality for the energies and for
    the AVERAGE map, equality or the exp-derived bound behind the bilateral table and the softmax."""
    from shinestacker_amd import DepthMapStack
    tag, h, w, float_type, kw = case
    FT = np.float64 if float_type == "float-64" else np.float32
    rng = np.random.default_rng(900 + [c[0] for c in STEP_CASES].index(tag))
    frames = scene(rng, 2, h, w, u16) + blocks(rng, 1, h, w, u16)
    gray = np.stack([oracle.bgr2gray_int(f) for f in frames]).astype(FT)
    dms = DepthMapStack(float_type=float_type, **kw)
    try:
        got = dms.get_sobel_map(gray)
        assert same_planes(got, np.stack([dmo.sobel_energy(g, FT) for g in gray])), (tag, "sobel")
        got = dms.get_laplacian_map(gray)
        en = np.stack([dmo.laplacian_energy(g, kw.get("blur_size", 5), kw.get("kernel_size", 5), FT) for g in gray])
        assert same_planes(got, en), (tag, "laplacian", dev(got, en))
        en = en / en.max()
        smooth = kw.get("smooth_size", 15)
        mt = kw.get("map_type", "average")

        def held(got, want_of, what):
            want = want_of(0)
            assert got.dtype == want.dtype and got.shape == want.shape, (tag, what)
            if np.array_equal(got, want):
                print(f"PATHS step {tag} {what} equal")
                return
            spread = max(dev(want_of(u), want) for u in (1, -1))
            print(f"PATHS step {tag} {what} dev={dev(got, want)} spread={spread}")
            assert dev(got, want) <= 2 * spread, (tag, what, dev(got, want), 2 * spread)
            assert (tag, what) in STEP_EXP_BOUND, (tag, what, "was bit-equal on the MI355X when this was measured")
        if smooth > 0:
            sm = dms.smooth_energy(en)
            held(sm, lambda u: np.stack([dmo.bilateral_f32(e.astype(np.float32), smooth, 25, 25, exp_ulp=u) for e in en]), "smoothed")
            en = np.stack([dmo.bilateral_f32(e.astype(np.float32), smooth, 25, 25) for e in en])
        fm = dms.get_focus_map(en)
        if mt == "average":
            assert same_planes(fm, np.stack(dmo.focus_map(list(en), mt)[0])), (tag, "focus map")
        else:
            held(fm, lambda u: np.stack(dmo.focus_map(list(en), mt, kw.get("temperature", 0.1), exp_ulp=u)[0]), "focus map")
    finally:
        dms.close()
