"""GPU: the AUTOMATIC level-pair plan of MI_ARITH_SEPARABLE (pair_levels = 0, csrc/tiled_host.hpp sep_pair_plan) -- the plan
of the benchmarked job.  A batch of SEP_PAIR_MIN_FRAMES = 192 float-32 frames or more runs levels (0, 1) as a pair
(level_sep_pair, level_sep_e, then the pair's payload: tile by tile -- level_sep_pl -- when both levels ran unchunked and the
batch holds at most 256 frames, else sep_payload_pair0 / 1, which fold the frame chunks' partial maxima); levels 2 and deeper
run unpaired, in frame chunks where they have few tiles.  Shorter batches and 8- / 16-bit frames never pair.

Every stack is bit-exact against oracle.StreamingOracle (arith="separable") on every tap, and every stack's profiler launch
counts equal those of the plan it claims (expected_launches).  Where levels 0 and 1 run in frame chunks (the small stacks)
the two plans launch equally many kernels, so there the counts pin the batch split but not the pairing; the mid-size stacks
(levels 0 and 1 unchunked: the pair's tile-by-tile pass adds launches) prove the pairing, the threshold included, and so
does the full-size job (tests/test_gpu_fullsize.py).  Every stack names pair_levels=0, so that the SHINESTACKER_AMD_PAIR_LEVELS
override of test runs cannot change the plan.  The frames are float-32 holding the generator's
8-bit values, as bench.py feeds them, with half of every frame noise (flagged and unflagged tiles of the tile-by-tile pass)."""
import numpy as np
import pytest

from test_gpu_separable import compare as compare_taps

pytestmark = pytest.mark.gpu


def compare(*args, **kw):
    """every tap, the base level's included (test_gpu_separable.compare)"""
    return compare_taps(*args, base=True, **kw)


SEP_PAIR_MIN_FRAMES = 192   # csrc/tiled_host.hpp
TH, TW = 28, 56             # separable tile: MI_SEP_TH x SepGeom::TW
SEP_LAUNCH_FRAMES = 16
H, W = 133, 201             # odd at every level, every tile a border tile (min_size=8: 4 levels + a 9 x 13 base)


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


def cdiv(a, b):
    return -(-a // b)


def tdiv(a, b):             # C++ integer division of a possibly negative int (toward zero)
    return a // b if a >= 0 else -(-a // b)


def level_tiles(h, w):
    return cdiv(w, TW) * cdiv(h, TH)


def chunk_frames(nb, tiles):
    """level_chunk_frames: (frames per chunk or per launch, whether the chunks run side by side)"""
    c = 3072 // max(tiles, 1)
    if not (c > 1 and nb >= 32):
        return min(nb, SEP_LAUNCH_FRAMES), False
    return min(SEP_LAUNCH_FRAMES, max(16, cdiv(cdiv(nb, c), 4) * 4)), True


def level_launches(h, w, nb, payload_tiles=False):
    """(border launches, interior launches, chunked) of one launch_level_sep call -- its level_walk / launch_walk -- over a
    batch of `nb` frames of an h x w level.  The interior launch takes the edge tiles too (levels of 16 x 16 and more) except the rows / columns at an odd
    far edge; chunked levels are one launch (blockIdx.y = chunk), the others consecutive launches of 16 frames;
    `payload_tiles` (PM = 3, level_sep_pl): one launch over the whole batch."""
    if h >= 16 and w >= 16:
        iy0 = ix0 = 0
        iy1 = max(0, (h - 6) // TH * TH) if h & 1 else cdiv(h, TH) * TH
        ix1 = max(0, (w - 6) // TW * TW) if w & 1 else cdiv(w, TW) * TW
    else:
        iy0, ix0 = cdiv(6, TH) * TH, cdiv(6, TW) * TW
        iy1, ix1 = tdiv(h - 6, TH) * TH, tdiv(w - 6, TW) * TW
    nyi, nxi = ((iy1 - iy0) // TH, (ix1 - ix0) // TW) if iy1 > iy0 and ix1 > ix0 else (0, 0)
    nborder = level_tiles(h, w) - nyi * nxi
    fc, chunked = chunk_frames(nb, level_tiles(h, w))
    nlaunch = 1 if payload_tiles or chunked else cdiv(nb, fc)
    return nlaunch * (nborder > 0), nlaunch * (nyi > 0), chunked and not payload_tiles


def expected_launches(shapes, batches):
    """The profiler's launch counts after `batches` = [(frames, paired), ...], derived from run_batch / launch_level_sep
    and the frame walk it shares with launch_level (level_walk / launch_walk, csrc/tiled_host.hpp).  Per batch:
      level 0 (level_sep, or level_sep_pair when paired): border launches -> PROF_LEVEL, interior launches -> PROF_LEVEL0;
        unpaired, its payload pass (sep_payload, which also folds the chunk partials: no merge_chunks) -> PROF_LEVEL;
      level l >= 1 (level_sep, or level_sep_e for the second level of a pair): border + interior launches -> PROF_LEVEL, then
        l = 1 of a pair: the pair's payload -> PROF_LEVEL: level_sep_pl over level 0's tiles (its border + interior launch)
          + sep_payload_pair0 + sep_payload_pair1 when levels 0 and 1 ran unchunked and the batch holds <= 256 frames, else
          sep_payload_pair0 + sep_payload_pair1 (2, as many as the two sep_payload passes of the unpaired plan);
        any other level: its payload pass (sep_payload) -> PROF_LEVEL;
      the base level: one scope -> PROF_BASE.
    So the plans differ in their counts only where the tile-by-tile pass runs."""
    n = {"level0": 0, "level": 0, "base": 0}
    nlev = len(shapes) - 1
    for nb, paired in batches:
        b0, i0, ch0 = level_launches(*shapes[0], nb)
        n["level"] += b0
        n["level0"] += i0
        if not paired:
            n["level"] += 1
        for lv in range(1, nlev):
            b, i, ch = level_launches(*shapes[lv], nb)
            n["level"] += b + i
            if lv == 1 and paired:
                if not ch0 and not ch and nb <= 256:
                    bt, it, _ = level_launches(*shapes[0], nb, payload_tiles=True)
                    k = bt + it + 2
                else:
                    k = 2
                n["level"] += k
            else:
                n["level"] += 1
        n["base"] += 1
    return n


def launches(L, st):
    return {k: st.profile_get(v)[1] for k, v in (("level0", L.PROF_LEVEL0), ("level", L.PROF_LEVEL), ("base", L.PROF_BASE))}


def assert_plan(L, st, batches, proves_pairing=True):
    """the batches ran as claimed: the counts are exactly those of the claimed plan.  `proves_pairing`: the claim is one the
    counts can refute (the same batches with every pairing flipped give other counts); False where levels 0 and 1 of the
    paired batches run in frame chunks, where the counts pin the batch split and each level's launches, not the pairing"""
    want = expected_launches(st.shapes, batches)
    flipped = expected_launches(st.shapes, [(nb, not p) for nb, p in batches])
    if proves_pairing:
        assert want != flipped, (batches, want)
    got = launches(L, st)
    assert got == want, f"plan {batches}: launch counts {got}, the claimed plan gives {want}, the flipped one {flipped}"


def make_frame(oracle, h, w, f, n, seed=7):
    """frame f of the n-frame generator stack (8-bit), its left half noise"""
    a = oracle.synth_frame_u8(h, w, f, n)
    a[:, : w // 2] = np.random.default_rng(seed * 100003 + f).integers(0, 256, (h, w // 2, 3), dtype=np.uint8)
    return a


def small_frames(oracle, n, gen_n=None):
    """n frames of H x W, some copied onto later ones across frame-chunk boundaries (exact ties: the first maximum wins,
    inside the pair's levels and inside the chunked levels after them)"""
    frames = [make_frame(oracle, H, W, f, gen_n or n) for f in range(n)]
    fc, chunked = chunk_frames(min(n, 256), level_tiles(H, W))
    assert chunked and fc == 16
    for dst, src in ((9, 4), (fc, fc - 1), (3 * fc + 5, 5), (7 * fc, 2 * fc), (11 * fc - 1, fc + 2), (n - 1, 3 * fc + 5)):
        frames[dst] = frames[src].copy()
    return frames


def upload(L, frames, dtype=np.float32):
    fb = frames[0].size * np.dtype(dtype).itemsize
    buf = L.DeviceBuffer(fb * len(frames))
    for i, f in enumerate(frames):
        buf.upload(f.astype(dtype), i * fb)
    return buf, fb


def oracle_of(oracle, frames, h=H, w=W, min_size=8):
    so = oracle.StreamingOracle(h, w, frames[0].dtype, min_size=min_size, arith="separable", keep_gauss=False)
    for f in frames:
        so.push_frame(f)
    return so, [g.copy() for g in so.gaussians(frames[-1])]


def sep_stack(L, pl=0, dtype=np.float32, h=H, w=W, min_size=8, **kw):
    st = L.Stack(h, w, in_dtype=dtype, out_dtype=np.uint16 if dtype == np.uint16 else np.uint8, arith="separable",
                 min_size=min_size, pair_levels=pl, **kw)
    st.profile()
    return st


@pytest.mark.parametrize("n", [SEP_PAIR_MIN_FRAMES, SEP_PAIR_MIN_FRAMES - 1])
def test_auto_pair_threshold(L, oracle, n):
    """one device push of 192 float-32 frames pairs levels (0, 1), one of 191 does not; both equal the oracle, and so do the
    same frames with pair_levels=2 (unpaired).  Levels 0 and 1 run in frame chunks here, where both plans launch equally
    many kernels: the mid-size test below proves the threshold from the counts."""
    frames = small_frames(oracle, n, SEP_PAIR_MIN_FRAMES)
    so, gs = oracle_of(oracle, frames)
    buf, _ = upload(L, frames)
    st = sep_stack(L)
    assert st.levels == 4
    st.push_frames_device(buf.ptr, n)
    assert_plan(L, st, [(n, n >= SEP_PAIR_MIN_FRAMES)], proves_pairing=False)
    compare(L, st, so, gs)
    st.close()
    st = sep_stack(L, pl=2)
    st.push_frames_device(buf.ptr, n)
    assert_plan(L, st, [(n, False)], proves_pairing=False)
    compare(L, st, so, gs)
    st.close()
    buf.free()


def test_auto_pair_interleaved_indices(L, oracle):
    """the 192-frame stack as rank 1 of 3 interleaved shards (set_first_index(1, 3), the bench's shard layout): the pair's
    payload passes look the winners up by the handle's own numbering from first_index; after export_indices every index tap
    and both base twins are 1 + 3 * the oracle's index, every other tap is the oracle's"""
    n = SEP_PAIR_MIN_FRAMES
    frames = small_frames(oracle, n)
    so, gs = oracle_of(oracle, frames)
    buf, _ = upload(L, frames)
    st = sep_stack(L)
    st.set_first_index(1, 3)
    st.push_frames_device(buf.ptr, n)
    assert_plan(L, st, [(n, True)], proves_pairing=False)
    st.export_indices(-1)
    compare(L, st, so, gs, index=lambda i: 1 + 3 * i)
    st.close()
    buf.free()


def test_auto_pair_several_paired_batches(L, oracle):
    """576 frames in one push: tiled_push cuts them into three batches of 192, every one paired -- the per-batch buffer
    sets alternate 0, 1, 0, and each batch waits for the previous one's payload and level-0 passes"""
    n = 3 * SEP_PAIR_MIN_FRAMES
    frames = small_frames(oracle, n)
    frames[400] = frames[100].copy()     # ties across batches
    frames[575] = frames[191].copy()
    so, gs = oracle_of(oracle, frames)
    buf, _ = upload(L, frames)
    st = sep_stack(L)
    st.push_frames_device(buf.ptr, n)
    assert_plan(L, st, [(SEP_PAIR_MIN_FRAMES, True)] * 3, proves_pairing=False)
    compare(L, st, so, gs)
    st.close()
    buf.free()


def test_auto_pair_paired_and_unpaired_batches_in_one_stack(L, oracle):
    """one handle, device pushes of 200 (paired), 40 (unpaired, levels in frame chunks), 192 (paired), 20 (unpaired,
    unchunked): the state and the kept-frame tap pass between the plans.  Then host frames with batch_frames=192: the
    staging ring's flush after 192 frames makes a paired batch, finish() flushes the last 8 unpaired."""
    pushes = [200, 40, 192, 20]
    n = sum(pushes)
    frames = small_frames(oracle, n)
    frames[230] = frames[150].copy()
    frames[440] = frames[235].copy()
    so, gs = oracle_of(oracle, frames)
    buf, fb = upload(L, frames)
    st = sep_stack(L)
    f0 = 0
    for k in pushes:
        st.push_frames_device(buf.ptr + f0 * fb, k)
        f0 += k
    assert_plan(L, st, [(k, k >= SEP_PAIR_MIN_FRAMES) for k in pushes], proves_pairing=False)
    compare(L, st, so, gs)
    st.close()
    buf.free()
    host = [f.astype(np.float32) for f in frames[:200]]
    so, gs = oracle_of(oracle, frames[:200])
    st = sep_stack(L, batch_frames=SEP_PAIR_MIN_FRAMES)
    for f in host:
        st.push_frame(f)
    compare(L, st, so, gs)
    assert_plan(L, st, [(SEP_PAIR_MIN_FRAMES, True), (8, False)], proves_pairing=False)
    st.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_auto_pair_is_float32_only(L, oracle, dtype):
    """192 frames of 8- or 16-bit input with pair_levels=0: no pair runs (the automatic pair measured slower there), and the
    result equals the oracle"""
    n = SEP_PAIR_MIN_FRAMES
    frames = small_frames(oracle, n)
    if dtype == np.uint16:
        frames = [f.astype(np.uint16) * 257 for f in frames]
    so, gs = oracle_of(oracle, frames)
    buf, _ = upload(L, frames, dtype)
    st = sep_stack(L, dtype=dtype)
    st.push_frames_device(buf.ptr, n)
    assert_plan(L, st, [(n, False)], proves_pairing=False)
    compare(L, st, so, gs)
    st.close()
    buf.free()


def test_auto_pair_benchmark_layout_at_mid_size(L, oracle):
    """the 24 MP job's layout at 0.42 of its pixels: 2912 x 3472 float-32 frames, levels 0 and 1 with more than 1536 tiles
    each (unchunked: the pair's payload takes the tile-by-tile pass), levels 2+ in frame chunks.  192 frames in one push;
    then, on the same buffer, 320 frames with batch_frames=320 -- one paired batch above 256 frames, whose payload is the
    per-quad kernels without chunks; frames 192-319 repeat frames 0-127 (exact ties across the two halves of the batch).
    batch_frames is named for every stack, so that the plan does not depend on the device memory free at the time.  ~39 GB.
    The launch counts prove the plan at the threshold: 192 frames pair (the tile-by-tile pass launches), the same frames
    with pair_levels=2 and 191 frames do not (the 320-frame batch launches as many kernels paired as unpaired)."""
    h, w, n0, n1 = 2912, 3472, SEP_PAIR_MIN_FRAMES, 320
    assert level_tiles(h // 2, w // 2) > 1536 and not chunk_frames(n1, level_tiles(h // 2, w // 2))[1]
    assert chunk_frames(n0, level_tiles(h // 4, w // 4))[1]
    fb = h * w * 3 * 4
    buf = L.DeviceBuffer(fb * n1)
    so = oracle.StreamingOracle(h, w, np.uint8, arith="separable", keep_gauss=False)
    for f in range(n0):
        a = make_frame(oracle, h, w, f, n0)
        buf.upload(a.astype(np.float32), f * fb)
        so.push_frame(a)
    gs = [g.copy() for g in so.gaussians(a)]
    L.check(L.load().mi_memcpy_d2d(0, buf.ptr + n0 * fb, buf.ptr, (n1 - n0) * fb))
    st = sep_stack(L, h=h, w=w, min_size=32, batch_frames=n0)
    assert st.levels == 6
    st.push_frames_device(buf.ptr, n0)
    assert_plan(L, st, [(n0, True)])
    auto = launches(L, st)
    compare(L, st, so, gs)
    st.close()
    st = sep_stack(L, pl=2, h=h, w=w, min_size=32, batch_frames=n0)
    st.push_frames_device(buf.ptr, n0)
    assert_plan(L, st, [(n0, False)])
    assert launches(L, st) != auto
    compare(L, st, so, gs)
    st.close()
    st = sep_stack(L, h=h, w=w, min_size=32, batch_frames=n0)
    st.push_frames_device(buf.ptr, n0 - 1)
    assert_plan(L, st, [(n0 - 1, False)])
    st.close()
    for f in range(n1 - n0):
        a = make_frame(oracle, h, w, f, n0)
        so.push_frame(a)
    gs = [g.copy() for g in so.gaussians(a)]
    st = sep_stack(L, h=h, w=w, min_size=32, batch_frames=n1)
    st.push_frames_device(buf.ptr, n1)
    assert_plan(L, st, [(n1, True)], proves_pairing=False)
    compare(L, st, so, gs)
    st.close()
    buf.free()
