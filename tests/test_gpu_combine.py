"""GPU: the local kernels of the winners-only combine (mi_combine_winner / _plan / _pack / _unpack) against their torch
statements on the same tensors, for a simulated world of three ranks, and Combiner.combine_winners() under RCCL with one
rank (fresh process: torch's HIP runtime has to be loaded before libmi355stack.so)."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SCRIPT = r'''
import os, sys
import numpy as np
import torch, torch.distributed as dist
torch.cuda.init()
sys.path.insert(0, os.getcwd())
from shinestacker_amd import _lib as L
from shinestacker_amd.multigpu import Combiner, TorchWinnerOps, first_max_rank
dist.init_process_group("nccl", rank=0, world_size=1)
dev = torch.device("cuda", 0)
st = L.Stack(200, 296)
hip, ref = Combiner(st), TorchWinnerOps()
g = torch.Generator(device="cpu").manual_seed(3)
# worlds 3 / 5 / 8 use one / two 64-bit words of packed per-rank counts in the block scan, 13 / 16 all four
for n, world in ((1, 3), (1023, 3), (1024, 3), (1025, 3), (300007, 3), (70001, 5), (262144, 8), (99999, 13), (131077, 16), (4099, 2)):
    cand = torch.randint(0, 50, (world, n), generator=g).float().to(dev)     # many exact ties
    if world == 8:
        cand[5] = 100.0 + torch.arange(n, device=dev) % 7                     # one rank wins whole 1024-pixel blocks
    win = hip.winner(cand)
    assert torch.equal(win, first_max_rank(cand)), n
    plan, totals = hip.plan(win, world)
    assert totals == ref.plan(win, world)[1] and sum(totals) == n
    for width in (1, 3):
        arr = torch.rand(n * width, generator=g).to(dev)
        packs = [hip.pack(win, plan, world, r, arr, width, totals[r]) for r in range(world)]
        for r in range(world):
            assert torch.equal(packs[r], ref.pack(win, None, world, r, arr, width, totals[r])), (n, width, r)
        # rank 1 receives the rows of ranks 0 and 2 into an array that holds its own rows already
        for me in range(world):
            mine = torch.where((win == me).repeat_interleave(width), arr, torch.full_like(arr, -1.0))
            want = mine.clone()
            bufs = [None if r == me else packs[r] for r in range(world)]
            hip.unpack(win, plan, world, me, bufs, mine, width)
            ref.unpack(win, None, world, me, bufs, want, width)
            assert torch.equal(mine, want) and torch.equal(mine, arr), (n, width, me)
# the whole protocol with one rank: nothing to exchange, the stack's result is unchanged; sync_level(0) then sync
rng = np.random.default_rng(5)
frames = [rng.integers(0, 256, (200, 296, 3), dtype=np.uint8) for _ in range(5)]
for arith in ("exact", "separable"):
    a = L.Stack(200, 296, arith=arith)
    for f in frames: a.push_frame(f)
    want = a.finish()
    b = L.Stack(200, 296, arith=arith)
    for f in frames: b.push_frame(f)
    Combiner(b).combine_winners()
    assert np.array_equal(b.finish(), want)
dist.destroy_process_group()
print("WINNERS_OK")
'''


def test_winner_kernels_and_protocol_world_1():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", SCRIPT], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert "WINNERS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


TWO_RANKS = r'''
import os, sys, json
import numpy as np
import torch, torch.distributed as dist
torch.cuda.init()
sys.path.insert(0, os.getcwd())
from shinestacker_amd import _lib as L
from shinestacker_amd.multigpu import Combiner, HostStagedComm
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)      # ONE GPU for both processes: RCCL refuses that
H, W, N = 300, 452, 12
rng = np.random.default_rng(17)
frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
frames[7] = frames[1].copy()      # the same frame on both ranks: exact ties across ranks, the lower global index must win
frames[9] = frames[4].copy()
frames[3] = frames[1].copy()      # ... and inside one rank
per = N // world
for arith in ("exact", "separable"):
    st = L.Stack(H, W, arith=arith)
    st.set_first_index(rank * per)
    for f in frames[rank * per:(rank + 1) * per]:
        st.push_frame(f)
    cb = Combiner(st, comm=HostStagedComm(dist.group.WORLD))      # the library's HIP kernels, not TorchWinnerOps
    assert type(cb).winner is Combiner.winner
    cb.combine_winners(with_index=True, root_energy=True)
    if rank == 0:
        whole = L.Stack(H, W, arith=arith)
        for f in frames:
            whole.push_frame(f)
        for lv in range(st.levels):
            for tap in (L.TAP_ENERGY, L.TAP_INDEX, L.TAP_FUSED_LAP):
                assert np.array_equal(st.tap(tap, lv), whole.tap(tap, lv)), (arith, lv, tap)
        assert np.array_equal(st.finish(), whole.finish()), arith
        whole.close()
        print("TIMINGS", arith, json.dumps(cb.timings))
    # the image alone needs the winners' Laplacians / base pixels only
    st2 = L.Stack(H, W, arith=arith)
    st2.set_first_index(rank * per)
    for f in frames[rank * per:(rank + 1) * per]:
        st2.push_frame(f)
    Combiner(st2, comm=HostStagedComm(dist.group.WORLD)).combine_winners(with_index=False, root_energy=False)
    if rank == 0:
        ref = L.Stack(H, W, arith=arith)
        for f in frames:
            ref.push_frame(f)
        assert np.array_equal(st2.finish(), ref.finish()), arith
        ref.close()
    st.close(); st2.close()
# INTERLEAVED shards (rank r holds frames r, r + world, ...: set_first_index(r, world)): the rank order is not the frame order
# any more, ties go by the global frame index -- frame 6 (rank 0) repeats frame 5 (rank 1): 5 must win although its rank is higher
frames[6] = frames[5].copy()
for arith in ("exact", "separable"):
    for kw in (dict(with_index=True, root_energy=True), dict(with_index=False, root_energy=False)):
        st = L.Stack(H, W, arith=arith)
        st.set_first_index(rank, world)
        for f in frames[rank::world]:
            st.push_frame(f)
        Combiner(st, comm=HostStagedComm(dist.group.WORLD)).combine_winners(**kw)
        if rank == 0:
            whole = L.Stack(H, W, arith=arith)
            for f in frames:
                whole.push_frame(f)
            if kw["with_index"]:
                for lv in range(st.levels):
                    for tap in (L.TAP_ENERGY, L.TAP_INDEX, L.TAP_FUSED_LAP):
                        assert np.array_equal(st.tap(tap, lv), whole.tap(tap, lv)), ("interleaved", arith, lv, tap)
                for tap in (L.TAP_BASE_IDX_E, L.TAP_BASE_IDX_D):
                    assert np.array_equal(st.tap(tap, st.levels), whole.tap(tap, st.levels)), ("interleaved", arith, tap)
            assert np.array_equal(st.finish(), whole.finish()), ("interleaved", arith)
            whole.close()
        st.close()
# a rank's own view: the index taps show global frame numbers, and an exported handle takes no more frames until reset
st = L.Stack(H, W, arith="separable")
st.set_first_index(rank, world)
for f in frames[rank::world]:
    st.push_frame(f)
own = st.tap(L.TAP_INDEX, 0)
assert set(np.unique(own)) <= set(range(rank, N, world))
try:
    st.push_frame(frames[0])
    raise SystemExit("push after export did not fail")
except RuntimeError:
    pass
st.reset()
st.push_frame(frames[0])
st.close()
dist.barrier()
dist.destroy_process_group()
if rank == 0:
    print("TWO_RANKS_OK")
'''


def test_device_combine_with_two_ranks_on_one_gpu(tmp_path):
    """`Combiner.combine_winners` with world == 2 and the library's HIP kernels (mi_combine_winner / plan / pack / unpack on
    the device-resident slabs): two processes share the one GPU, the collectives travel over gloo through the host
    (`HostStagedComm`) because RCCL refuses two ranks on one device.  Cross-rank duplicate frames: the first maximum in
    global frame order must win (pyramid.py:48-55).  Both arithmetics, both exchange variants; contiguous frame blocks and
    interleaved shards (set_first_index(rank, world): ties by the global frame index, mi_combine_winner_idx)."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    script = tmp_path / "two_ranks.py"
    script.write_text(TWO_RANKS)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)],
                       env=env, capture_output=True, text=True, timeout=900,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert "TWO_RANKS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


FORCED = r'''
import os, sys, json
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, os.getcwd())
from shinestacker_amd import _lib as L
from shinestacker_amd.multigpu import Combiner
rng = np.random.default_rng(5)
frames = [rng.integers(0, 256, (200, 296, 3), dtype=np.uint8) for _ in range(5)]
a = L.Stack(200, 296, arith="separable")
for f in frames: a.push_frame(f)
want = a.finish()
b = L.Stack(200, 296, arith="separable")
for f in frames: b.push_frame(f)
cb = Combiner(b, force=True)
cb.combine_winners()
assert np.array_equal(b.finish(), want)
assert set(cb.timings) == {"wait_level0_ms", "exchange_level0_ms", "wait_rest_ms", "exchange_rest_ms"}
print("FORCED_OK", json.dumps(cb.timings))
'''


def test_forced_combine_at_world_1_runs_the_kernels_and_changes_nothing():
    """bench.py's `combine_ms`: the per-rank kernel work of the exchange (winner map, plan, pack, unpack) run on a single
    rank's own rows -- nothing moves, the result is unchanged, the phases are timed."""
    r = subprocess.run([sys.executable, "-c", FORCED], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert "FORCED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_flow_with_two_ranks_on_one_gpu(scaling):
    """bench.py's multi-rank path end to end on ONE GPU (MI_BENCH_ONE_GPU=1: both ranks on device 0, collectives staged
    through the host over gloo): frame sharding with global indices, the device combine kernels, rank 0's collapse, the
    max-over-ranks timing and the verification of the result against the oracle fed ALL frames."""
    import json
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MI_BENCH_ONE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--frames", "8", "--height", "600",
                        "--width", "900", "--steps", "1", "--warmup", "1", "--scaling", scaling, "--full", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=root)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["verified"] is True, d
    assert d["combine_ms"] > 0 and "SHARING ONE GPU" in d["config"]["parallelism"]


MANY_RANKS = r'''
import os, sys
import numpy as np
import torch, torch.distributed as dist
torch.cuda.init()
sys.path.insert(0, os.getcwd())
from shinestacker_amd import _lib as L
from shinestacker_amd.multigpu import Combiner, HostStagedComm
from oracle import oracle as orc
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)      # every rank on device 0: RCCL refuses that
comm = HostStagedComm(dist.group.WORLD)
H, W = 264, 360                   # 3 levels + a 33 x 45 base
FULL, PAYLOAD = dict(with_index=True, root_energy=True), dict(with_index=False, root_energy=False)
fails = []


def make_frames(n, seed, hi=256, lo=0, band=True):
    rng = np.random.default_rng(seed)
    fr = [rng.integers(lo, hi, (H, W, 3)).astype(np.uint16 if hi > 256 else np.uint8) for _ in range(n)]
    if band:
        for f in fr:
            f[96:160] = (lo + hi) // 3    # flat in every frame: energy exactly 0 there, the frame index alone decides
    return fr


def shard(n, layout):
    """(global frame indices of this rank, first index, index stride)"""
    if layout == "interleaved":
        return list(range(rank, n, world)), rank, world
    sizes = [n // world + (r >= world - n % world) for r in range(world)]     # ragged contiguous blocks
    a = sum(sizes[:rank])
    return list(range(a, a + sizes[rank])), a, 1


def push(st, frames, idx, dtype, how):
    data = [frames[k].astype(dtype) for k in idx]
    if not data:
        return
    if how == "host":
        for f in data:
            st.push_frame(f)
        return
    fb = data[0].nbytes
    stride = fb + 4096            # frames apart in device memory: push_frames_device with a frame stride
    buf = L.DeviceBuffer(stride * len(data))
    for k, f in enumerate(data):
        buf.upload(f, k * stride)
    st.push_frames_device(buf.ptr, len(data), stride)
    st.sync()
    buf.free()


def check(name, st, frames, kw, dtype, arith, gen, pl):
    """rank 0 after the combine == one handle that pushed every frame == the oracle of every frame, bit for bit"""
    whole = L.Stack(H, W, in_dtype=dtype, arith=arith, gen_kernel=gen, pair_levels=pl)
    for f in frames:
        whole.push_frame(f.astype(dtype))
    so = orc.StreamingOracle(H, W, frames[0].dtype, arith=arith, gen_kernel=gen, keep_gauss=False)
    for f in frames:
        so.push_frame(f)
    taps = [(L.TAP_FUSED_LAP, lv, so.best_lap[lv]) for lv in range(st.levels)]
    if kw["root_energy"]:
        taps += [(L.TAP_ENERGY, lv, so.best_e[lv]) for lv in range(st.levels)]
    if kw["with_index"]:
        taps += [(L.TAP_INDEX, lv, so.best_idx[lv]) for lv in range(st.levels)]
        taps += [(L.TAP_BASE_IDX_E, st.levels, so.idx_e), (L.TAP_BASE_IDX_D, st.levels, so.idx_d)]
    for tap, lv, want in taps:
        got, ref = st.tap(tap, lv), whole.tap(tap, lv)
        if not np.array_equal(got, ref):
            fails.append(f"{name}: tap {tap} level {lv} differs from the whole stack at {int((got != ref).sum())} values")
        if not np.array_equal(got, want):
            fails.append(f"{name}: tap {tap} level {lv} differs from the oracle at {int((got != want).sum())} values")
    got, ref, want = st.finish(), whole.finish(), so.finish()
    if not np.array_equal(got, ref):
        fails.append(f"{name}: finish() differs from the whole stack at {int((got != ref).sum())} values")
    if not np.array_equal(got, want):
        fails.append(f"{name}: finish() differs from the oracle at {int((got != want).sum())} values")
    fb = st.tap(L.TAP_FUSED_BASE)
    if not (np.array_equal(fb, whole.tap(L.TAP_FUSED_BASE)) and np.array_equal(fb, so.fused_base())):
        fails.append(f"{name}: fused base differs")
    whole.close()


def local(name, frames, layout, dtype, arith, how):
    """every rank's OWN state right after its push == the oracle of its shard (global indices): the per-GPU half of the
    protocol, with every rank's process on the one GPU at once and every handle fresh (its slabs zeroed at creation: that
    zeroing must be complete before the first frame's kernels write them)"""
    idx, first, stride = shard(len(frames), layout)
    bad = []
    if idx:
        st = L.Stack(H, W, in_dtype=dtype, arith=arith)
        st.set_first_index(first, stride)
        push(st, frames, idx, dtype, how)
        so = orc.StreamingOracle(H, W, frames[0].dtype, arith=arith, keep_gauss=False)
        for k in idx:
            so.push_frame(frames[k])
        g = lambda a: first + a * stride
        taps = [(t, lv, want) for lv in range(st.levels)
                for t, want in ((L.TAP_ENERGY, so.best_e[lv]), (L.TAP_INDEX, g(so.best_idx[lv])), (L.TAP_FUSED_LAP, so.best_lap[lv]))]
        taps += [(L.TAP_BASE_IDX_E, st.levels, g(so.idx_e)), (L.TAP_BASE_IDX_D, st.levels, g(so.idx_d))]
        for tap, lv, want in taps:
            got = st.tap(tap, lv)
            if not np.array_equal(got, want):
                bad.append(f"{name}: rank {rank} ({len(idx)} frames) tap {tap} level {lv} differs at {int((got != want).sum())} values")
        st.close()
    every = [None] * world
    dist.all_gather_object(every, bad)
    if rank == 0:
        fails.extend(sum(every, []))
        print("CASE", name, flush=True)


def run(name, frames, layout, proto, kw, dtype=np.uint8, arith="exact", how="host", gen=0.4, pl=0, handle=None):
    """one stack sharded over the ranks; `handle`: (Stack, Combiner) of an earlier stack, reset and reused"""
    idx, first, stride = shard(len(frames), layout)
    if handle is None:
        st = L.Stack(H, W, in_dtype=dtype, arith=arith, gen_kernel=gen, pair_levels=pl)
        handle = (st, Combiner(st, comm=comm))     # the library's HIP kernels, not TorchWinnerOps
    st, cb = handle
    st.reset()
    st.set_first_index(first, stride)
    push(st, frames, idx, dtype, how)
    if proto == "combine":
        cb.combine(**kw)
    else:
        cb.combine_winners(**kw)
    if rank == 0:
        check(name, st, frames, kw, dtype, arith, gen, pl)
        print("CASE", name, flush=True)
    return handle


N = 13                            # ragged at both worlds: blocks of 1 / 2 at world 8, 4 / 5 at world 3
dup = make_frames(N, 1)
dup[2] = dup[1].copy()            # contiguous: inside rank 0 at world 3, across ranks at world 8 ...
dup[N - 1] = dup[1].copy()        # ... and from the last rank
ilv = make_frames(N, 2)
ilv[world] = ilv[world - 1].copy()    # interleaved: frame W - 1 on rank W - 1, its copy W on rank 0 -- the lower index must win
ilv[1 + world] = ilv[1].copy()        # the same rank (1) twice
ilv16 = make_frames(N, 3, hi=65536)
ilv16[world] = ilv16[world - 1].copy()
fewg = make_frames(min(5, world - 1), 6)     # fewer frames than ranks, on FRESH handles: their zeroed slabs would beat the
                                             # negative winning energies of gen_kernel=0.7 unless the empty ranks withdraw
# (name, frames, layout, protocol, variant, dtype, arith, push, gen_kernel, pair_levels): input types and pushes rotate
cases = [
    ("combine/full/exact/u8/host/contiguous", dup, "contiguous", "combine", FULL, np.uint8, "exact", "host", 0.4, 0),
    ("combine/payload/separable/u16/host/interleaved", ilv16, "interleaved", "combine", PAYLOAD, np.uint16, "separable", "host", 0.4, 0),
    ("combine/full/separable/f32/host/interleaved", ilv, "interleaved", "combine", FULL, np.float32, "separable", "host", 0.4, 0),
    ("combine/full/exact/u16/device/interleaved/gen0.7", ilv16, "interleaved", "combine", FULL, np.uint16, "exact", "device", 0.7, 0),
    ("combine/payload/exact/u8/host/interleaved/gen0.7/few", fewg, "interleaved", "combine", PAYLOAD, np.uint8, "exact", "host", 0.7, 0),
    ("winners/full/separable/f32/device/interleaved/pair_levels=1", ilv, "interleaved", "winners", FULL, np.float32, "separable", "device", 0.4, 1),
    ("winners/payload/exact/u8/host/contiguous", dup, "contiguous", "winners", PAYLOAD, np.uint8, "exact", "host", 0.4, 0),
    ("winners/full/exact/u16/host/interleaved", ilv16, "interleaved", "winners", FULL, np.uint16, "exact", "host", 0.4, 0),
    ("winners/payload/separable/u8/device/interleaved/gen0.7", ilv, "interleaved", "winners", PAYLOAD, np.uint8, "separable", "device", 0.7, 0),
    ("winners/full/exact/u8/host/interleaved/gen0.7/few", fewg, "interleaved", "winners", FULL, np.uint8, "exact", "host", 0.7, 0),
]
# each rank's own stack first: one host frame per rank on three ranks at world 8 (dup, contiguous), one or two elsewhere
for name, frames, layout, dtype, arith, how in (("local/exact/u8/host/contiguous", dup, "contiguous", np.uint8, "exact", "host"),
                                                 ("local/exact/u16/host/interleaved", ilv16, "interleaved", np.uint16, "exact", "host"),
                                                 ("local/separable/u8/host/contiguous", dup, "contiguous", np.uint8, "separable", "host")):
    local(name, frames, layout, dtype, arith, how)
for name, frames, layout, proto, kw, dtype, arith, how, gen, pl in cases:
    st, _ = run(name, frames, layout, proto, kw, dtype, arith, how, gen, pl)
    st.close()
# handle reuse: one Stack and one Combiner per rank run three stacks back to back, reset in between, each in another layout.
# The first two are full-range noise (high energies); the last holds low-contrast frames only, fewer frames than ranks, so the
# ranks past its frames push nothing and their slabs still hold the previous stack's state -- which must not win anything.
loud = make_frames(N, 4, band=False)
few = make_frames(min(5, world - 1), 5, lo=100, hi=132)
for proto, dtype, arith, how, kws in (("winners", np.uint8, "exact", "host", (FULL, FULL, FULL)),
                                      ("combine", np.float32, "separable", "device", (PAYLOAD, FULL, FULL))):
    h = None
    for k, (frames, layout) in enumerate(((loud, "contiguous"), (ilv, "interleaved"), (few, "interleaved"))):
        h = run(f"reuse/{proto}/{arith}/stack{k}/{layout}/{len(frames)} frames", frames, layout, proto, kws[k], dtype, arith, how,
                handle=h)
    assert h[0].frames_pushed == (1 if rank < len(few) else 0)
    h[0].close()
dist.barrier()
if rank == 0:
    for f in fails:
        print("FAIL", f)
    print(f"MANY_RANKS_OK {world}" if not fails else f"MANY_RANKS_FAILED {len(fails)}")
dist.destroy_process_group()
'''


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("world", [3, 8])
def test_whole_protocol_with_many_ranks_on_one_gpu(tmp_path, world):
    """`Combiner.combine()` and `Combiner.combine_winners()` with 3 and 8 ranks, every rank a process on the one GPU (gloo +
    `HostStagedComm`): rank 0's every tap and its image == one handle that pushed all frames == the oracle, bit for bit.
    Both protocols in the full and the payload-only variant, both arithmetics, 8- / 16-bit and float-32 frames, host and
    strided device pushes, ragged contiguous and interleaved shards, ties across and inside ranks, a flat band, negative
    taps, the forced level pair, fresh handles on ranks without frames; then handles reused across stacks, the last with
    fewer frames than ranks.  First every rank's own state right after its push, against the oracle of its shard."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    script = tmp_path / "many_ranks.py"
    script.write_text(MANY_RANKS)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)],
                       env=env, capture_output=True, text=True, timeout=1100,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-6000:])
    assert f"MANY_RANKS_OK {world}" in r.stdout, r.stdout[-6000:] + r.stderr[-4000:]
