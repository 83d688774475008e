"""GPU: the tail of a separable stack -- everything behind level 0 -- against oracle.StreamingOracle(arith="separable"), bit
for bit and on every tap (each level's energy, arg-max and fused Laplacian, the base level's arg-max twins and fused base, the
collapsed and the final image).

Round 7 changed how the pair's tile-by-tile payload pass (level_sep_pl, csrc/kernels_sep.hpp) gets what it consumes: the
winners' G_l pixels come from the staged patch in LDS (float-32 interior tiles and all border tiles; 8- / 16-bit interior
tiles still read them from memory), the tile's window of G_{l+2} is loaded once per step ahead of the next winner's prefetch
and shared through LDS, and the G_{l+1} patch of float-32 interior tiles is split over the patch's halo rows and X.  The
arithmetic and the walk order did not change, so every tap must stay equal to the oracle:

  * small stacks (420 x 620, 421 x 619, 1000 x 1500; float-32 and 8-bit; pair_levels 0 / 1 / 2; one batch, batches of 3 and
    a resident push long enough for frame chunks): the levels behind level 0 in every launch shape, the pair's per-quad
    payload kernels, chunk partials folded by the payload passes;
  * stacks large enough for levels 0 and 1 to run unchunked (the tile-by-tile pass), float-32 and 8-bit, whose tiles have
    exactly one winner (`single`), a handful (`coherent`, the generator: 2 to 9 at 36 frames, median 5), more than 32 (`noise`: flagged, left to the per-quad
    kernels) and both kinds side by side (`mixed`), as tests/test_gpu_pair.py::test_pair_tile_payload builds them.

The one-launch forms of the small levels, the base and the collapse that the same round considered were not built: there is no
second path to choose between here, the cases above run the only one."""
import numpy as np
import pytest

from test_gpu_separable import compare as compare_taps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


def compare(L, st, so):
    return compare_taps(L, st, so, base=True)


def oracle_of(oracle, frames, **kw):
    h, w = frames[0].shape[:2]
    so = oracle.StreamingOracle(h, w, np.uint8, arith="separable", keep_gauss=False, **kw)
    for f in frames:
        so.push_frame(f)
    return so


def upload(L, frames, dt):
    fb = frames[0].size * np.dtype(dt).itemsize
    buf = L.DeviceBuffer(fb * len(frames))
    for i, f in enumerate(frames):
        buf.upload(f.astype(dt), i * fb)
    return buf


@pytest.mark.parametrize("pl", [0, 1, 2])
@pytest.mark.parametrize("dt", [np.float32, np.uint8])
@pytest.mark.parametrize("h,w", [(420, 620), (421, 619), (1000, 1500)])
def test_tail_small_stacks(L, oracle, h, w, dt, pl):
    """7 frames pushed from the host in one batch and in batches of 3, then 40 frames resident in one push (32 or more: the
    levels with few tiles run in frame chunks); frames 2 and 33 repeat frame 0 (the first maximum wins)"""
    n = 40
    frames = [oracle.synth_frame_numpy(h, w, f, n) for f in range(n)]
    frames[2] = frames[0].copy()
    frames[33] = frames[0].copy()
    for batch in (0, 3):
        so = oracle_of(oracle, frames[:7], min_size=16)
        st = L.Stack(h, w, in_dtype=dt, arith="separable", batch_frames=batch, pair_levels=pl, min_size=16)
        for f in frames[:7]:
            st.push_frame(f.astype(dt))
        compare(L, st, so)
        st.close()
    so = oracle_of(oracle, frames, min_size=16)
    buf = upload(L, frames, dt)
    st = L.Stack(h, w, in_dtype=dt, arith="separable", pair_levels=pl, min_size=16)
    st.push_frames_device(buf.ptr, n)
    compare(L, st, so)
    st.close()
    buf.free()


TILE_H, TILE_W, TILE_N = 2912, 3472, 36
_tile_cache = {}


def tile_stack(oracle, kind):
    """(frames, oracle) of one kind of winner pattern, built once for both input types"""
    if kind not in _tile_cache:
        _tile_cache.clear()      # one kind at a time: 36 frames of 10 MP and the oracle's state
        h, w, n = TILE_H, TILE_W, TILE_N
        rng = np.random.default_rng(11)
        if kind == "noise":
            frames = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]
        elif kind == "single":
            # one frame in focus everywhere, the others flat: every tile of levels 0 and 1 has that one winner (or, where the
            # sharp frame has no energy either, frame 0: the first maximum)
            frames = [np.full((h, w, 3), 90 + f, np.uint8) for f in range(n)]
            frames[5] = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        else:
            frames = [oracle.synth_frame_numpy(h, w, f, n) for f in range(n)]
            if kind == "mixed":
                for f in frames:
                    f[:, : w // 2] = rng.integers(0, 256, (h, w // 2, 3)).astype(np.uint8)
        _tile_cache[kind] = (frames, oracle_of(oracle, frames))
    return _tile_cache[kind]


def winners_per_tile(idx, th=28, tw=56):
    """distinct arg-max values of every whole th x tw tile of a level-0 index image"""
    h, w = idx.shape
    t = idx[: h // th * th, : w // tw * tw].reshape(h // th, th, w // tw, tw).transpose(0, 2, 1, 3).reshape(-1, th * tw)
    t = np.sort(t, axis=1)
    return 1 + (np.diff(t, axis=1) != 0).sum(axis=1)


@pytest.mark.parametrize("dt", [np.float32, np.uint8])
@pytest.mark.parametrize("kind", ["single", "coherent", "mixed", "noise"])
def test_tail_tile_payload_winners(L, oracle, kind, dt):
    """levels 0 and 1 unchunked and forced into a pair: the payload is the tile-by-tile pass.  The winner counts per tile the
    case is named for are checked on the oracle's level-0 arg-max before the comparison."""
    frames, so = tile_stack(oracle, kind)
    per_tile = winners_per_tile(so.best_idx[0])
    if kind == "single":
        assert np.median(per_tile) == 1 and per_tile.max() <= 2
    elif kind == "coherent":
        assert 2 <= np.median(per_tile) <= 16 and per_tile.max() <= 32
    elif kind == "noise":
        assert per_tile.min() > 32
    else:
        assert per_tile.min() <= 16 and per_tile.max() > 32
    buf = upload(L, frames, dt)
    st = L.Stack(TILE_H, TILE_W, in_dtype=dt, arith="separable", pair_levels=1)
    st.push_frames_device(buf.ptr, TILE_N)
    compare(L, st, so)
    st.close()
    buf.free()
