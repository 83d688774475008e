"""CPU, gloo, worlds 2 / 3 / 5 / 8: every combine protocol of shinestacker_amd/multigpu.py against the oracle of the WHOLE
stack, bit for bit.

One process group per world runs every scenario: each rank builds the running state of its shard with the oracle (standing
in for the per-GPU HIP path, indices mapped to global frame numbers), the ranks combine with the product's protocols, and
rank 0 must hold exactly the state of all frames pushed in one go -- every level's energy, index and fused Laplacian, both
base twins (energy, index, winner's base pixel) and the fused base.  Scenarios: contiguous blocks of ragged sizes,
interleaved shards (rank order != frame order: ties go by global index), fewer frames than ranks (ranks with no frames
offer hostile slabs through `withdraw_candidates`), duplicate frames across and inside ranks, a flat band (energy 0 in
every frame: the index alone decides), negative kernel taps (gen_kernel=0.7), and a 2 x 3 frame whose state is smaller
than the world (empty pixel chunks)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

WORLDS = (2, 3, 5, 8)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _scenarios(world):
    """name -> (frames, shards [global frame indices per rank], StreamingOracle keywords)"""
    rng = np.random.default_rng(1000 + world)
    H, W = 40, 56

    def frames(n, h=H, w=W, dtype=np.uint8, band=True):
        hi = 256 if dtype == np.uint8 else 65536
        fr = [rng.integers(0, hi, (h, w, 3), dtype=dtype) for _ in range(n)]
        if band:
            for f in fr:
                f[12:28] = hi // 3      # flat in every frame: Laplacian and deviation exactly 0, the index decides
        return fr

    def contiguous(n):       # ragged blocks: the later ranks take one frame more, ranks beyond n take none
        sizes = [n // world + (r >= world - n % world) for r in range(world)]
        cuts = np.cumsum([0] + sizes)
        return [list(range(cuts[r], cuts[r + 1])) for r in range(world)]

    def interleaved(n):
        return [list(range(r, n, world)) for r in range(world)]

    sc = {}
    nc = {2: 7, 3: 11, 5: 13, 8: 19}[world]            # blocks of 2 to 4 frames, never all of one size
    fr = frames(nc)
    fr[nc - 2] = fr[1].copy()                           # contiguous: the lower index on the lower rank, another rank
    fr[2] = fr[1].copy()                                # ... and one inside rank 0
    sc["contiguous"] = (fr, contiguous(nc), {})
    n = 2 * world + 3                                   # 7, 9, 13, 19: every rank holds 2 or 3 frames
    fr = frames(n)
    fr[world] = fr[world - 1].copy()                    # frame W lives on rank 0, its earlier copy W - 1 on rank W - 1
    fr[world + 1 + world] = fr[world + 1].copy()        # the same rank (1) twice
    sc["interleaved"] = (fr, interleaved(n), {})
    sc["interleaved_separable"] = (fr, interleaved(n), {"arith": "separable"})
    fr = frames(n, dtype=np.uint16)
    fr[world + 1] = fr[world - 1].copy()                # frame W + 1 on rank 1, W - 1 on rank W - 1
    sc["interleaved_gen07_u16"] = (fr, interleaved(n), {"gen_kernel": 0.7})   # negative taps: negative winning energies
    few = {2: 1, 3: 2, 5: 3, 8: 5}[world]               # fewer frames than ranks: ranks few.. push nothing
    fr = frames(few)
    sc["few_interleaved"] = (fr, interleaved(few), {})
    sc["few_contiguous"] = (fr, [[r] if r < few else [] for r in range(world)], {})
    # ties between DIFFERENT payloads: per-frame states with energies in {-1, 0, 1} and a payload of their own -- a wrong
    # tie-break or a gather of the wrong row shows in the payloads and the fused base, not only in the indices
    syn = _synthetic_frames(world, n)
    sc["synthetic_interleaved"] = (syn, interleaved(n), {"synthetic": True})
    sc["synthetic_contiguous"] = (syn, contiguous(n), {"synthetic": True})
    sc["synthetic_few_interleaved"] = (syn[:few], interleaved(few), {"synthetic": True})
    fr = frames(world + 2, 2, 3, band=False)            # no pyramid level, 12 state pixels: chunks of rank >= 6 are empty
    fr[world] = fr[world - 1].copy()
    sc["tiny_interleaved"] = (fr, interleaved(world + 2), {})
    return sc


def _synthetic_frames(world, n, sizes=(96, 24, 6, 6)):
    """n frames' own states (two levels + the base twins): energies with many exact ties, payloads distinct per frame"""
    rng = np.random.default_rng(7 + world)
    return [[(rng.integers(-1, 2, m).astype(np.float32), rng.standard_normal(3 * m).astype(np.float32)) for m in sizes]
            for _ in range(n)]


def _first_max(syn, ks):
    """the state of the frames `ks` (ascending global indices) pushed in order: np.argmax's first maximum per pixel"""
    out = []
    for lv in range(len(syn[ks[0]])):
        e = np.stack([syn[k][lv][0] for k in ks])
        best = np.argmax(e, axis=0)
        ar = np.arange(e.shape[1])
        lap = np.stack([syn[k][lv][1].reshape(-1, 3) for k in ks])[best, ar].ravel()
        out.append((e[best, ar], lap, np.asarray(ks, np.int32)[best]))
    return out


def _levels(so, first=0, step=1):
    """(energy, payload, global index) of every level and both base twins of a StreamingOracle; local frame k -> first + k * step"""
    g = lambda a: np.asarray(first + a * step, np.int32)
    hb, wb = so.shapes[so.levels]
    yy, xx = np.mgrid[0:hb, 0:wb]
    bases = np.stack(so.bases)
    out = [(so.best_e[lv], so.best_lap[lv], g(so.best_idx[lv])) for lv in range(so.levels)]
    out.append((so.b_ent, bases[so.idx_e, yy, xx], g(so.idx_e)))
    out.append((so.b_dev, bases[so.idx_d, yy, xx], g(so.idx_d)))
    return [tuple(np.ascontiguousarray(a, dt).ravel() for a, dt in zip(t, (np.float32, np.float32, np.int32))) for t in out]


def _rank_state(orc, frames, shard, kw, inter, world):
    if kw.get("synthetic"):
        sizes = [e.size for e, _ in frames[0]]
    else:
        h, w = frames[0].shape[:2]
        so = orc.StreamingOracle(h, w, frames[0].dtype, min_size=8, **kw)
        hb, wb = so.shapes[so.levels]
        sizes = [a * b for a, b in so.shapes[:so.levels]] + [hb * wb, hb * wb]
    if not shard:   # a rank with no frames: hostile slab contents, which the withdrawal must neutralise
        return [(np.full(m, 1e30, np.float32), np.full(3 * m, 7.0, np.float32), np.zeros(m, np.int32)) for m in sizes], True
    if kw.get("synthetic"):
        return _first_max(frames, shard), False
    for k in shard:
        so.push_frame(frames[k])
    return _levels(so, shard[0], world if inter else 1), False


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    fails = []
    try:
        from oracle import oracle as orc
        from shinestacker_amd import multigpu as mg
        grp = dist.group.WORLD
        for name, (frames, shards, kw) in _scenarios(world).items():
            inter = "interleaved" in name
            mine, empty = _rank_state(orc, frames, shards[rank], kw, inter, world)
            want = None
            if rank == 0 and kw.get("synthetic"):
                want = _first_max(frames, list(range(len(frames))))
                fused_want = (((0.0 + want[-2][1]) + want[-1][1]) / 2.0).astype(np.float32)
            elif rank == 0:
                h, w = frames[0].shape[:2]
                so = orc.StreamingOracle(h, w, frames[0].dtype, min_size=8, **kw)
                for f in frames:
                    so.push_frame(f)
                want = _levels(so)
                fused_want = so.fused_base().ravel()

            def fresh():
                t = [tuple(torch.from_numpy(a.copy()) for a in lv) for lv in mine]
                if empty:
                    for e, _, i in t:
                        mg.withdraw_candidates(e, i)
                return t

            def check(proto, got, index=True, energy=True):
                if rank != 0:
                    return
                for lv, ((e, lp, ix), (we, wl, wi), orig) in enumerate(zip(got, want, mine)):
                    for what, a, b, live in (("energy", e, we, energy), ("lap", lp, wl, True), ("index", ix, wi, index)):
                        b = b if live else orig[("energy", "lap", "index").index(what)]   # a variant that leaves it stale
                        if not np.array_equal(np.asarray(a), b):
                            bad = int((np.asarray(a) != b).sum())
                            fails.append(f"world {world} {name} {proto}: state {lv} {what} differs at {bad} of {b.size}"
                                         + ("" if live else " (must be untouched)"))
                be, bd = np.asarray(got[-2][1]), np.asarray(got[-1][1])      # the winners' base pixels, both twins
                if not np.array_equal((((0.0 + be) + bd) / 2.0).astype(np.float32), fused_want):
                    fails.append(f"world {world} {name} {proto}: fused base differs")

            # combine_state, level by level
            t = fresh()
            for e, lp, ix in t:
                mg.combine_state(e, lp, ix, grp, mg.torch_select, tiebreak_index=inter)
            check("combine_state", t)
            # combine_all: a list of states (packed) and one flat slab (in place), all four variants
            for wi in (True, False):
                for re in (True, False):
                    var = dict(with_index=wi, root_energy=re)
                    t = fresh()
                    mg.combine_all(t, grp, mg.torch_select, tiebreak_index=inter, **var)
                    check(f"combine_all {var}", t, wi, re)
                    t = fresh()
                    slab = [tuple(torch.cat([lv[k] for lv in t]) for k in range(3))]
                    mg.combine_all(slab, grp, mg.torch_select, tiebreak_index=inter, **var)
                    check(f"combine_all slab {var}", _split(slab[0], t), wi, re)
                    # combine_winners in Combiner.combine_winners' two phases: level 0, then the rest
                    t = fresh()
                    e, lp, ix = (torch.cat([lv[k] for lv in t]) for k in range(3))
                    n0 = t[0][0].numel() if len(t) > 2 else 0
                    ops = mg.TorchWinnerOps()
                    mg.combine_winners(e[:n0], lp[:3 * n0], ix[:n0], grp, ops, tiebreak_index=inter, **var)
                    mg.combine_winners(e[n0:], lp[3 * n0:], ix[n0:], grp, ops, tiebreak_index=inter, **var)
                    check(f"combine_winners {var}", _split((e, lp, ix), t), wi, re)
        if rank == 0:
            ret["fails"] = fails
    finally:
        dist.destroy_process_group()


def _split(flat, like):
    """a flat (e, lap, idx) back into the per-state pieces of `like`"""
    out, off = [], 0
    for e, _, _ in like:
        m = e.numel()
        out.append((flat[0][off:off + m], flat[1][3 * off:3 * (off + m)], flat[2][off:off + m]))
        off += m
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", WORLDS)
def test_every_protocol_at_world_equals_whole_stack(oracle, world):
    port = _free_port()
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
        fails = list(ret["fails"])
    assert not fails, "\n".join(fails[:40]) + f"\n({len(fails)} mismatches)"


def test_scenarios_cover_what_they_claim():
    """the layouts really are what the scenario names say: empty ranks, empty pixel chunks, cross-rank ties whose lower
    index lives on the higher rank"""
    from shinestacker_amd.multigpu import chunk_bounds
    for world in WORLDS:
        sc = _scenarios(world)
        for name, (frames, shards, _) in sc.items():
            assert sorted(sum(shards, [])) == list(range(len(frames))), name
        assert any(not s for s in sc["few_interleaved"][1]) and any(not s for s in sc["few_contiguous"][1])
        assert len({len(s) for s in sc["contiguous"][1]}) == 2        # ragged blocks
        fr, shards, _ = sc["interleaved"]
        rank_of = {k: r for r, s in enumerate(shards) for k in s}
        assert np.array_equal(fr[world], fr[world - 1]) and rank_of[world - 1] > rank_of[world]
        assert np.array_equal(fr[2 * world + 1], fr[world + 1]) and rank_of[2 * world + 1] == rank_of[world + 1]
    assert any(a == b for a, b in chunk_bounds(2 * 3, 8)) and any(a == b for a, b in chunk_bounds(2 * 2 * 3, 8))
