"""GPU: float-32 frames that are NOT small integers, against oracle.StreamingOracle, bit for bit.

Every other float-32 frame of the suite holds integers in 0 ... 255 (uint8.astype(float32), the generator).  With such
frames every partial sum of the level-0 reduce of MI_ARITH_SEPARABLE (integer taps 20 k, one final * float32(1/400)) is an
integer below 2^24, exact in any order: a changed association in the float-32 level-0 code (level_sep / level_sep_pair and
their payload passes, csrc/kernels_sep.hpp) gives the same bits; the float32(k), rs = 1 branch of red_taps never meets a
float-32 frame; and the finish (clip, abs, truncate) and the energies never see a value a uint8 stack could not produce.
The frames here have full 24-bit mantissas (`frac255`, `unit`), leave the output range on both sides (`wide`), make
Q = lap^2 subnormal (`tiny`) and are scaled by powers of two (`pow2`: a reference-free scaling property on top of the
oracle comparison).  Each generator's defining condition is asserted on the frames / on the oracle's taps, so that an edit
cannot quietly turn a case back into integers.

Compared, with tests/test_gpu_separable.py::compare: every level's energy, arg-max and fused Laplacian, the base level's
arg-max twins and fused base, the kept frame's Gaussians, the collapsed and the finished image -- all np.array_equal.

NaN and Inf are left out: the reference defines no behaviour for them and the outcome of the oracle's `>` chain on them is an
accident.  Float-32 frames enter through Stack (and the classes built on it) only: the aligning pipeline
(pipeline.align_and_stack_device and its relatives) takes 8- and 16-bit frames, so there is no product entry point to cover
here."""
import numpy as np
import pytest

from test_gpu_separable import compare as compare_taps
from test_gpu_auto_pair import SEP_PAIR_MIN_FRAMES, assert_plan, chunk_frames, level_tiles, sep_stack
from test_gpu_auto_pair import H as AUTO_H, W as AUTO_W
from test_gpu_tail import upload

pytestmark = pytest.mark.gpu

N = 7                       # frames of the small stacks; frame N - 1 repeats frame N - 3
SIZES = [(420, 620), (421, 619), (284, 458), (131, 259)]
SCALING_SIZE = (284, 458)   # the one size of `tiny` and `pow2`
TINY = 2.0 ** -70
POW2 = (-20, 20)


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


# ------------------------------------------------------------------------------------------------ frames
def box_blur(img, r):
    """mean over (2 r + 1)^2 neighbours, edges replicated (float64)"""
    p = np.pad(img, ((r, r), (r, r), (0, 0)), mode="edge")
    c = np.cumsum(np.cumsum(p, axis=0), axis=1)
    c = np.pad(c, ((1, 0), (1, 0), (0, 0)))
    k = 2 * r + 1
    return (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)


_scene_cache = {}


def default_dups(n):
    return ((n - 1, n - 3),)


def scene(h, w, n=N, seed=0, dups=None):
    """n float64 frames of one h x w scene, every value in [0, 254) with a random fraction (so that value / 255 stays below 1 in float32): a blocky texture with many dark and
    many bright blocks plus fine detail, sharp in the frame's own band of rows and blended towards its blur elsewhere (weight
    2^-distance, the distance in sevenths of the stack), so that the arg-max changes from band to band.  `dups` = ((dst, src), ...): frame dst is a copy of the earlier
    frame src (exact ties: the first must win); default ((n - 1, n - 3),)."""
    dups = tuple(dups or default_dups(n))
    key = (h, w, n, seed, dups)
    if key not in _scene_cache:
        if len(_scene_cache) > 12:
            _scene_cache.clear()
        rng = np.random.default_rng([seed, h, w, n])
        coarse = rng.integers(0, 255, (h // 6 + 2, w // 6 + 2, 3)).astype(np.float64)
        kind = rng.random(coarse.shape[:2])
        coarse[kind < 0.3] = rng.integers(0, 6, coarse.shape)[kind < 0.3]          # dark blocks
        coarse[kind > 0.8] = rng.integers(246, 254, coarse.shape)[kind > 0.8]      # bright blocks
        amp = np.where((kind < 0.3) | (kind > 0.8), 8, 40)[:, :, None]     # (finer detail there: the blocks stay dark / bright)
        grow = np.ones((6, 6, 1))
        sharp = np.kron(coarse, grow)[:h, :w] + np.rint(rng.uniform(-1, 1, (h, w, 3)) * np.kron(amp, grow)[:h, :w])
        sharp = np.clip(sharp, 0, 253)
        blur = box_blur(sharp, 3)
        band = np.arange(h) * n // h
        frames = []
        for f in range(n):
            wgt = (0.5 ** (np.abs(band - f) * min(1.0, N / n)))[:, None, None]
            v = np.floor(wgt * sharp + (1 - wgt) * blur)          # the integer texture, 0 ... 253
            frames.append(v + rng.random((h, w, 3)))              # + a uniform fraction: < 254, a full mantissa
        for dst, src in dups:
            assert src < dst
            frames[dst] = frames[src].copy()
        _scene_cache[key] = frames
    return _scene_cache[key]


def gen_frac255(h, w, **kw):
    return [f.astype(np.float32) for f in scene(h, w, **kw)]


def gen_unit(h, w, **kw):
    return [(f / 255.0).astype(np.float32) for f in scene(h, w, **kw)]


def gen_wide(h, w, **kw):
    return [(f * (73000.0 / 255.0) - 3000.0).astype(np.float32) for f in scene(h, w, **kw)]


def gen_tiny(h, w, **kw):
    return [f * np.float32(TINY) for f in gen_frac255(h, w, **kw)]


def gen_pow2(h, w, k, **kw):
    return [f * np.float32(2.0 ** k) for f in gen_frac255(h, w, **kw)]


GEN = {"frac255": gen_frac255, "unit": gen_unit, "wide": gen_wide, "tiny": gen_tiny,
       "pow2-20": lambda h, w, **kw: gen_pow2(h, w, -20, **kw), "pow2+20": lambda h, w, **kw: gen_pow2(h, w, 20, **kw)}


def check_frames(name, frames, dups=None):
    """the generator's own condition, on the frames"""
    a = np.stack(frames)
    assert a.dtype == np.float32 and np.isfinite(a).all()
    if name == "frac255":
        assert a.min() >= 0 and a.max() <= 255 and (a == np.rint(a)).mean() < 0.01
        assert (np.frexp(a)[0] * 2.0 ** 24 % 2 == 1).mean() > 0.4       # the last mantissa bit is set on about half
    elif name == "unit":
        assert a.min() >= 0 and a.max() < 1 and (a == np.rint(a)).mean() < 0.01
    elif name == "wide":
        assert a.min() < -2900 and a.max() > 69000
        assert (a < 0).mean() >= 0.05 and (a > 255).mean() >= 0.05 and (a > 65535).mean() >= 0.01
    elif name == "tiny":
        assert np.array_equal(a.astype(np.float64) / TINY, np.stack(gen_frac255(*a.shape[1:3], n=len(frames), dups=dups)))
    for dst, src in dups or default_dups(len(frames)):
        assert np.array_equal(frames[dst], frames[src]) and not np.array_equal(frames[src], frames[src - 1])


def check_index(so, dups=None):
    """the index taps are not trivial, and a repeated frame never wins: its twin came first (and does win somewhere)"""
    idx = so.best_idx[0]
    dups = dups or default_dups(so.n)
    assert len(np.unique(idx)) >= 4 and np.isin(idx, [s for _, s in dups]).any() and not np.isin(idx, [d for d, _ in dups]).any()
    assert all(np.isfinite(e).all() for e in so.best_e) and all(np.isfinite(x).all() for x in so.best_lap)


TINIEST_NORMAL = np.finfo(np.float32).tiny


def check_tiny_energies(so):
    e = so.best_e[0]
    assert ((e > 0) & (e < TINIEST_NORMAL)).any(), "no level-0 energy is subnormal: the case proves nothing"
    assert all((x != 0).any() for x in so.best_e), "a level's energies are all zero"


_oracle_cache = {}


def reference(oracle, name, h, w, od, n=N, dups=None, **kw):
    """(frames, the oracle after all of them, the last frame's Gaussians), built once per case and left unchanged"""
    key = (name, h, w, np.dtype(od).name, n, dups, tuple(sorted(kw.items())))
    if key not in _oracle_cache:
        if len(_oracle_cache) > 24:
            _oracle_cache.clear()
        frames = GEN[name](h, w, n=n, dups=dups)
        check_frames(name, frames, dups)
        so = oracle.StreamingOracle(h, w, od, keep_gauss=False, **kw)
        for f in frames[:-1]:
            so.push_frame(f)
        so.keep_gauss = True
        gs = so.push_frame(frames[-1])
        check_index(so, dups)
        if name == "tiny":
            check_tiny_energies(so)
        _oracle_cache[key] = (frames, so, gs)
    return _oracle_cache[key]


def run(L, frames, device, od, **kw):
    h, w = frames[0].shape[:2]
    st = L.Stack(h, w, in_dtype=np.float32, out_dtype=od, **kw)
    st.resident = None
    if device:
        st.resident = upload(L, frames, np.float32)
        st.push_frames_device(st.resident.ptr, len(frames))
    else:
        for f in frames:
            st.push_frame(f)
    return st


def close(st):
    st.close()
    if st.resident is not None:
        st.resident.free()


def compare(L, st, so, gs=None):
    assert st.levels == so.levels
    compare_taps(L, st, so, gs, base=True)
    close(st)


# ------------------------------------------------------------------------------------------------ 1. separable
@pytest.mark.parametrize("pl", [0, 1, 2, 3])
@pytest.mark.parametrize("od", [np.uint8, np.uint16])
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("name", ["frac255", "unit", "wide"])
def test_separable_values(L, oracle, name, h, w, od, pl):
    """every level-0 variant of the separable arithmetic: both implementations, the forced pair plans (these stacks are below
    the automatic plan's threshold), one batch and batches of 3, host pushes and one resident push.  min_size=16: one level
    more than the default, pairs at two depths."""
    frames, so, gs = reference(oracle, name, h, w, od, arith="separable", min_size=16)
    for impl in (1, 2):
        for batch in (0, 3):
            for device in (False, True):
                st = run(L, frames, device, od, arith="separable", min_size=16, impl=impl, batch_frames=batch, pair_levels=pl)
                compare(L, st, so, gs)


@pytest.mark.parametrize("pl", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["tiny", "pow2-20", "pow2+20"])
def test_separable_scaled_values(L, oracle, name, pl):
    """subnormal Q = lap^2 (`tiny`: kept, not flushed -- near zero a flush flips arg-max ties) and frames scaled by 2^-20 / 2^20
    against the oracle"""
    h, w = SCALING_SIZE
    frames, so, gs = reference(oracle, name, h, w, np.uint8, arith="separable", min_size=16)
    for impl in (1, 2):
        for batch, device in ((0, False), (3, False), (0, True)):
            st = run(L, frames, device, np.uint8, arith="separable", min_size=16, impl=impl, batch_frames=batch, pair_levels=pl)
            compare(L, st, so, gs)


@pytest.mark.parametrize("pl", [0, 1, 2, 3])
@pytest.mark.parametrize("k", POW2)
def test_scaling_by_a_power_of_two_is_exact(L, oracle, k, pl):
    """reference-free: against the GPU's own run on the unscaled frames, frames * 2^k give the same arg-max, Laplacians * 2^k and
    energies * 2^(2k), exactly -- no operation of the path rounds differently when nothing overflows or underflows.  The same
    is asserted of the oracle first: it is what makes 2^k a fair choice for these frames."""
    h, w = SCALING_SIZE
    name = "pow2%+d" % k
    _, so1, _ = reference(oracle, "frac255", h, w, np.uint8, arith="separable", min_size=16)
    _, sok, _ = reference(oracle, name, h, w, np.uint8, arith="separable", min_size=16)
    s = np.float32(2.0 ** k)
    for lv in range(so1.levels):
        assert np.array_equal(sok.best_idx[lv], so1.best_idx[lv])
        assert np.array_equal(sok.best_lap[lv], so1.best_lap[lv] * s) and np.array_equal(sok.best_e[lv], so1.best_e[lv] * s * s)
    kw = dict(arith="separable", min_size=16, pair_levels=pl, batch_frames=3)
    a = run(L, gen_frac255(h, w), False, np.uint8, **kw)
    b = run(L, GEN[name](h, w), False, np.uint8, **kw)
    for lv in range(a.levels):
        assert np.array_equal(b.tap(L.TAP_INDEX, lv), a.tap(L.TAP_INDEX, lv)), f"index {lv}"
        assert np.array_equal(b.tap(L.TAP_FUSED_LAP, lv), a.tap(L.TAP_FUSED_LAP, lv) * s), f"lap {lv}"
        assert np.array_equal(b.tap(L.TAP_ENERGY, lv), a.tap(L.TAP_ENERGY, lv) * s * s), f"energy {lv}"
    close(a)
    close(b)


# ------------------------------------------------------------------------------------------------ 2. non-integral taps
@pytest.mark.parametrize("pl", [0, 1])
@pytest.mark.parametrize("min_size", [8, 16])
@pytest.mark.parametrize("a", [0.35, 0.7, 0.4])
@pytest.mark.parametrize("name", ["frac255", "wide"])
def test_separable_tap_kinds(L, oracle, name, a, min_size, pl):
    """gen_kernel 0.35: the float32(k), rs = 1 branch of red_taps; 0.7: integer taps with a negative outer one (energies can be
    negative); 0.4: the control"""
    rk = oracle.red_taps_f32(a)
    assert (rk[3] == 1) == (a == 0.35) and (rk[0] < 0) == (a == 0.7)
    h, w = (131, 259) if min_size == 8 else (284, 458)
    frames, so, gs = reference(oracle, name, h, w, np.uint8, arith="separable", min_size=min_size, gen_kernel=a)
    for impl in (1, 2):
        for batch, device in ((0, False), (3, False), (0, True)):
            st = run(L, frames, device, np.uint8, arith="separable", min_size=min_size, gen_kernel=a, impl=impl,
                     batch_frames=batch, pair_levels=pl)
            compare(L, st, so, gs)


# ------------------------------------------------------------------------------------------------ 3. exact arithmetic
@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("use_fma", [True, False])
@pytest.mark.parametrize("od", [np.uint8, np.uint16])
@pytest.mark.parametrize("name", ["frac255", "wide", "tiny"])
def test_exact_values(L, oracle, name, od, use_fma, impl):
    h, w = (421, 619) if od == np.uint8 else (131, 259)
    frames, so, gs = reference(oracle, name, h, w, od, min_size=16, use_fma=use_fma)
    for batch, device in ((0, False), (3, True)):
        st = run(L, frames, device, od, min_size=16, use_fma=use_fma, impl=impl, batch_frames=batch)
        compare(L, st, so, gs)


def ref_shaped_f64(oracle, frames, od, min_size, use_fma=True):
    """float_type='float-64' of the reference on float-32 frames, from oracle.RefShaped's steps (its stack() takes the output
    type from the frames).  The base level's gray -> histogram bin cast is clamped to the output type's range, the rule
    pyramid_oracle.c states for float-32 stacks (the reference's own .astype of a value outside the type is undefined): the
    features are taken of a gray surrogate base that truncates to the clamped bins."""
    r = oracle.RefShaped(min_size=min_size, float_type=np.float64, use_fma=use_fma)
    h, w = frames[0].shape[:2]
    pyrs = [r.laplacian_pyramid(f, int(np.log2(min(h, w) / min_size)))[0] for f in frames]
    nl = len(pyrs[0]) - 1
    top = np.iinfo(od).max
    ent, dev = [], []
    for p in pyrs:
        bins = np.clip(np.trunc(oracle.bgr2gray_f32(p[-1].astype(np.float32), use_fma)), 0, top)
        e, d = r.base_features(np.repeat((bins + 0.5)[:, :, None], 3, axis=2), od)
        ent.append(e)
        dev.append(d)
    be, bd = np.argmax(np.stack(ent), axis=0), np.argmax(np.stack(dev), axis=0)
    bases = np.stack([p[-1] for p in pyrs])
    yy, xx = np.indices(be.shape)
    lo, hi = np.minimum(be, bd), np.maximum(be, bd)
    fused = [None] * nl + [(0.0 + bases[lo, yy, xx] + bases[hi, yy, xx]) / 2]
    best, energy = [], []
    for lev in range(nl):
        fl, b, e = r.fuse_level(np.stack([p[lev] for p in pyrs]))
        fused[lev] = fl
        best.append(b)
        energy.append(e.max(axis=0))
    return fused, best, energy, be, bd, r.collapse(fused, top).astype(od)


@pytest.mark.parametrize("od", [np.uint8, np.uint16])
@pytest.mark.parametrize("name", ["frac255", "wide"])
def test_float64_values(L, oracle, name, od):
    """Stack takes float-32 frames with float_type MI_F64 (the one-frame-at-a-time float-64 kernels): float64 Laplacians, base and
    collapse, float32 energies"""
    h, w = 131, 259
    frames = GEN[name](h, w)
    check_frames(name, frames)
    fused, best, energy, be, bd, want = ref_shaped_f64(oracle, frames, od, 16)
    assert len(np.unique(best[0])) >= 4 and not (best[0] == N - 1).any()
    st = run(L, frames, False, od, min_size=16, float_type=L.MI_F64)
    assert st.levels == len(best)
    for lv in range(st.levels):
        assert np.array_equal(st.tap(L.TAP_INDEX, lv), best[lv]), f"index {lv}"
        assert np.array_equal(st.tap(L.TAP_ENERGY, lv), energy[lv]), f"energy {lv}"
        lap = st.tap(L.TAP_FUSED_LAP, lv)
        assert lap.dtype == np.float64 and np.array_equal(lap, fused[lv]), f"lap {lv}"
    assert np.array_equal(st.tap(L.TAP_BASE_IDX_E), be) and np.array_equal(st.tap(L.TAP_BASE_IDX_D), bd)
    got = st.finish()
    assert np.array_equal(st.tap(L.TAP_FUSED_BASE), fused[-1])
    assert got.dtype == want.dtype and np.array_equal(got, want)
    close(st)


# ------------------------------------------------------------------------------------------------ 4. the tail, the automatic plan
TAIL_N, TAIL_DUPS = 40, ((2, 0), (33, 0))


@pytest.mark.parametrize("pl", [0, 1, 2])
@pytest.mark.parametrize("name", ["frac255", "wide"])
def test_tail_values(L, oracle, name, pl):
    """tests/test_gpu_tail.py::test_tail_small_stacks' resident push -- 40 frames, 32 or more: the levels with few tiles run in
    frame chunks, whose partial maxima the payload passes fold; frames 2 and 33 repeat frame 0"""
    h, w = 420, 620
    frames, so, gs = reference(oracle, name, h, w, np.uint8, n=TAIL_N, dups=TAIL_DUPS, arith="separable", min_size=16)
    st = run(L, frames, True, np.uint8, arith="separable", min_size=16, pair_levels=pl)
    compare(L, st, so, gs)


FC = 16     # frames per chunk of the automatic-plan stack (test_gpu_auto_pair.small_frames)
AUTO_DUPS = ((9, 4), (FC, FC - 1), (3 * FC + 5, 5), (7 * FC, 2 * FC), (11 * FC - 1, FC + 2), (SEP_PAIR_MIN_FRAMES - 1, 3 * FC + 5))


@pytest.mark.parametrize("name", ["frac255", "wide"])
def test_auto_pair_values(L, oracle, name):
    """the automatic plan: one resident push of 192 float-32 frames pairs levels (0, 1) (level_sep_pair, level_sep_e, the
    per-quad payload kernels over frame chunks).  Frames repeat across chunk boundaries, and frame 112 repeats frame 32
    across the two halves of the batch."""
    n = SEP_PAIR_MIN_FRAMES
    assert chunk_frames(n, level_tiles(AUTO_H, AUTO_W)) == (FC, True)
    frames, so, gs = reference(oracle, name, AUTO_H, AUTO_W, np.uint8, n=n, dups=AUTO_DUPS, arith="separable", min_size=8)
    buf = upload(L, frames, np.float32)
    st = sep_stack(L)
    assert st.levels == so.levels == 4
    st.push_frames_device(buf.ptr, n)
    assert_plan(L, st, [(n, True)], proves_pairing=False)
    compare_taps(L, st, so, gs, base=True)
    st.close()
    buf.free()


# ------------------------------------------------------------------------------------------------ 5. unaligned device frames
@pytest.mark.parametrize("arith", ["exact", "separable"])
def test_unaligned_device_frames(L, oracle, arith):
    """(211, 333, offset 4, padding 12) of test_gpu_fuzz.py::test_device_frames_with_odd_alignment_and_stride: float-32 frames
    at a base address that is only 4-byte aligned, a frame stride larger than a frame -- where the staging's choice of vector
    or scalar loads could meet a rounding difference"""
    h, w, off, pad = 211, 333, 4, 12
    frames, so, gs = reference(oracle, "frac255", h, w, np.uint8, arith=arith)
    stride = frames[0].nbytes + pad
    buf = L.DeviceBuffer(off + stride * len(frames) + 64)
    for i, f in enumerate(frames):
        buf.upload(f, off + i * stride)
    for impl in (L.IMPL_TILED, L.IMPL_SIMPLE):
        st = L.Stack(h, w, in_dtype=np.float32, out_dtype=np.uint8, impl=impl, batch_frames=3, arith=arith)
        st.push_frames_device(buf.ptr + off, len(frames), stride)
        compare_taps(L, st, so, gs, base=True)
        st.close()
    buf.free()
