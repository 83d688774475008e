"""Calling the library from several threads at once: a runner, the jobs it runs and the job tables of test_gpu_threads.py.
A plain module shared by test_thread_cases_host.py, which checks the runner itself and the tables on the CPU, and
test_gpu_threads.py.  No device at import, seeded, NumPy only apart from the library calls inside the jobs.

A job is a name, prepare(), call(round), `expected` and release().  prepare() runs on the main thread before any worker
starts: it uploads, allocates and creates handles.  call(round) returns bytes; most jobs do the same thing every round, the
warp walks (below) another frame size.  `expected` is what the call must return, computed once, on the main thread, by the
restatements the single-thread tests hold the kernels to (warp_cases, stereo_restatement, lens_restatement,
demosaic_restatement, finish_restatement, depth_render_restatement, guided_restatement, features_restatement,
nlm_restatement, unsharp_restatement) and by the oracle for whole stacks -- never by a serial run of the library.
differing(got, round) counts the elements in which a result misses it: bytes for nearly every job, and for the three whose
single-thread tests state a tolerance (DepthMap: one count on 0.1 % of the values; the ECC estimate: 2e-3 px at the corners,
1e-5 in rho, one iteration per level; the feature estimate: rtol 1e-9) that tolerance, unchanged.

run_jobs() is what a test calls: every expected result, every prepare(), no buffer in two jobs, every job once on the main
thread (it must equal `expected` there, so that a failure under threads is a threading failure and nothing else), then
run_threads(), then every release() -- unless a thread is still alive, whose buffers must not be freed under it.

The warp walks.  The border blur's tile list and the affine warp's coordinate tables live in two process-wide caches keyed
by (device, stream) that only grow: a larger request waits for the stream, frees the buffer and allocates a larger one
(warp_scratch / warp_coord_scratch in csrc/capi.hip).  Four threads walk LADDER up and down, each by its own row of WALKS,
so that -- were the threads in step -- each of them is at some round the first to ask one of the two caches for more than
anybody has asked before, while the others have warps in flight; test_thread_cases_host.py checks the rows for that.  On the
null stream the four share one cache entry and one enqueue lock; on their own streams each grows its own.  The once-on-the-
main-thread call of a walk is its round 0, the smallest frame, so that the null stream's cache is not grown before the
threads start (frames warped earlier in the same process have grown it already: the file is meant to run on its own too).
"""
import ctypes as C
import functools
import threading
import time

import numpy as np

import warp_cases as wc

MAX_THREADS = 8
ROUNDS = 20
DEADLINE_S = 60.0


# ---------------------------------------------------------------------------------------------------------------- runner
class Report:
    """what run_threads saw: mismatches [(job name, round, differing elements)], errors [(job name, round, exception)],
    alive [job name] (threads that had not returned at the deadline), calls {job name: calls that returned}, overlapped
    {job name: how many of its calls ran while a call of another job was in progress -- a measure, printed with the result:
    threads that took turns would have tested nothing}, seconds"""

    def __init__(self, names):
        self.names = list(names)
        self.mismatches, self.errors, self.alive = [], [], []
        self.calls = {n: 0 for n in self.names}
        self.overlapped = {n: 0 for n in self.names}
        self.seconds = 0.0

    @property
    def ok(self):
        return not (self.mismatches or self.errors or self.alive)

    def __str__(self):
        parts = []
        if self.alive:
            parts.append("alive: [%s]" % ", ".join(self.alive))
        if self.errors:
            parts.append("errors: " + "; ".join("%s, round %d: %r" % e for e in self.errors))
        if self.mismatches:
            parts.append("mismatches: " + "; ".join("%s, round %d: %d differ" % m for m in self.mismatches[:12]))
            if len(self.mismatches) > 12:
                parts.append("... %d mismatches in all" % len(self.mismatches))
        return " | ".join(parts) or "ok: %s in %.3f s; calls beside another thread's: %s" % (self.calls, self.seconds, self.overlapped)


def run_threads(jobs, rounds, deadline_s):
    """One daemon thread per job, released together by a barrier; each calls its job `rounds` times and compares every
    result with the job's expected one.  A mismatch is recorded and the thread goes on; an exception is recorded, ends its
    thread and raises the stop flag, which every thread looks at before each call -- after an error nothing more is started.
    The main thread joins against one common deadline; threads alive then are reported and the flag is raised for them.
    Nothing is tried twice."""
    jobs = list(jobs)
    assert len({j.name for j in jobs}) == len(jobs), "job names must differ"
    report = Report(j.name for j in jobs)
    stop = threading.Event()
    barrier = threading.Barrier(len(jobs))
    spans = {j.name: [] for j in jobs}          # [start, end] of every call; end None while it runs

    def work(job):
        try:
            barrier.wait(timeout=deadline_s)
        except threading.BrokenBarrierError as e:
            report.errors.append((job.name, -1, e))
            stop.set()
            return
        for r in range(rounds):
            if stop.is_set():
                return
            span = [time.monotonic(), None]
            spans[job.name].append(span)
            try:
                got = job.call(r)
                span[1] = time.monotonic()
                bad = job.differing(got, r)
            except BaseException as e:  # noqa: BLE001  (reported, never swallowed: Report.ok is False)
                report.errors.append((job.name, r, e))
                stop.set()
                return
            report.calls[job.name] = r + 1
            if bad:
                report.mismatches.append((job.name, r, int(bad)))

    threads = [threading.Thread(target=work, args=(j,), name=j.name, daemon=True) for j in jobs]
    t0 = time.monotonic()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, t0 + deadline_s - time.monotonic()))
    report.alive = [t.name for t in threads if t.is_alive()]
    if report.alive:
        stop.set()
    report.seconds = time.monotonic() - t0
    ends = {n: [(a, b if b is not None else float("inf")) for a, b in list(v)] for n, v in spans.items()}
    for n, mine in ends.items():
        others = [s for m, v in ends.items() if m != n for s in v]
        report.overlapped[n] = sum(any(a < d and c < b for c, d in others) for a, b in mine)
    return report


def differing_elements(got, want, dtype=np.uint8):
    """how many elements of two byte strings differ; a length that differs counts whole"""
    if len(got) != len(want):
        return max(len(got), len(want), 1)
    if got == want:
        return 0
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if len(got) % np.dtype(dtype).itemsize == 0:
        a, b = a.view(dtype), b.view(dtype)
        if np.dtype(dtype).kind == "f":     # NaN payloads included
            a, b = a.view("u%d" % a.itemsize), b.view("u%d" % b.itemsize)
    return int((a != b).sum())


class Job:
    dtype = np.uint8        # the element type differing() counts in

    def __init__(self, name):
        self.name = name

    def prepare(self):
        pass

    def call(self, r):
        raise NotImplementedError

    def release(self):
        pass

    @functools.cached_property
    def expected(self):
        return self.want()

    def want(self):
        raise NotImplementedError

    def expected_at(self, r):
        return self.expected

    def differing(self, got, r):
        return differing_elements(got, self.expected_at(r), self.dtype)

    def buffers(self):
        """(address, bytes) of every buffer the job owns, once prepared"""
        return []

    def host_arrays(self):
        """the host arrays the job uploads or pushes"""
        return []


class FnJob(Job):
    """a job made of plain functions (the runner's own tests)"""

    def __init__(self, name, call, expected, prepare=None, release=None):
        super().__init__(name)
        self._call, self._want, self._prepare, self._release = call, expected, prepare, release

    def prepare(self):
        if self._prepare:
            self._prepare()

    def call(self, r):
        return self._call(r)

    def want(self):
        return self._want

    def release(self):
        if self._release:
            self._release()


class Sequence(Job):
    """two jobs on one thread, one after the other in every round"""

    def __init__(self, first, second):
        super().__init__(first.name + " + " + second.name)
        self.parts = (first, second)

    def prepare(self):
        for p in self.parts:
            p.prepare()

    def call(self, r):
        return tuple(p.call(r) for p in self.parts)

    def want(self):
        return tuple(p.expected for p in self.parts)

    def differing(self, got, r):
        return sum(p.differing(g, r) for p, g in zip(self.parts, got))

    def release(self):
        for p in self.parts:
            p.release()

    def buffers(self):
        return [b for p in self.parts for b in p.buffers()]

    def host_arrays(self):
        return [a for p in self.parts for a in p.host_arrays()]


def shared_buffers(jobs):
    """the pairs of jobs of which one owns a byte the other owns too"""
    spans = sorted((a, a + max(n, 1), j.name) for j in jobs for a, n in j.buffers())
    out, end, owner = [], 0, None
    for lo, hi, name in spans:
        if lo < end and name != owner:
            out.append((owner, name))
        if hi > end:
            end, owner = hi, name
    return out


def run_jobs(jobs, rounds=ROUNDS, deadline_s=DEADLINE_S):
    jobs = list(jobs)
    assert 1 <= len(jobs) <= MAX_THREADS, len(jobs)
    for j in jobs:
        j.expected          # on the main thread, before anything runs
    prepared, report = [], None
    try:
        for j in jobs:
            prepared.append(j)
            j.prepare()
        assert not shared_buffers(jobs), shared_buffers(jobs)
        alone = [(j.name, j.differing(j.call(0), 0)) for j in jobs]
        assert all(n == 0 for _, n in alone), ("differs from the restatement on the main thread, before any thread started", alone)
        report = run_threads(jobs, rounds, deadline_s)
        return report
    finally:
        if report is None or not report.alive:
            for j in reversed(prepared):
                j.release()


# -------------------------------------------------------------------------------------------------------- device helpers
class DeviceJob(Job):
    """a job with device buffers of its own, on the null stream or (`own_stream`) on the stream of a Stack(64, 64) handle
    of its own, which it synchronises instead of the device"""

    def __init__(self, L, name, own_stream=False):
        super().__init__(name)
        self.L, self.own_stream = L, own_stream
        self.stream, self.handle, self.bufs = None, None, []

    def open_stream(self):
        if self.own_stream:
            self.handle = self.L.Stack(64, 64)
            self.stream = self.handle.stream

    def put(self, arr):
        b = self.empty(arr.nbytes)
        b.upload(arr)
        return b

    def empty(self, nbytes):
        b = self.L.DeviceBuffer(nbytes)
        self.bufs.append(b)
        return b

    def wait(self):
        if self.handle is not None:
            self.handle.sync()
        else:
            self.L.check(self.L.load().mi_device_synchronize(0))

    def buffers(self):
        return [(b.ptr, b.nbytes) for b in self.bufs]

    def release(self):
        for b in self.bufs:
            b.free()
        self.bufs = []
        if self.handle is not None:
            self.handle.close()
            self.handle, self.stream = None, None


class FreeJob(DeviceJob):
    """one device-form entry point on resident buffers: `inputs` {key: array} are uploaded once, `outputs`
    [(key, shape, dtype)] are preset to 0xA5 once, launch(job) queues the call on job.stream with the addresses job.ptr[key];
    a call is launch, wait, download of every output.  want() -> the arrays the outputs must hold."""

    def __init__(self, L, name, inputs, outputs, launch, want, own_stream=False, dtype=np.uint8):
        super().__init__(L, name, own_stream)
        self.inputs, self.outputs, self.launch, self._want, self.dtype = inputs, outputs, launch, want, dtype
        self.ptr = {}

    def prepare(self):
        self.open_stream()
        for key, arr in self.inputs.items():
            self.ptr[key] = self.put(np.ascontiguousarray(arr)).ptr
        self.out = []
        for key, shape, dtype in self.outputs:
            b = self.put(np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xA5, np.uint8))
            self.ptr[key] = b.ptr
            self.out.append((b, shape, dtype))

    def call(self, r):
        self.launch(self)
        self.wait()
        return b"".join(b.download(shape, dtype).tobytes() for b, shape, dtype in self.out)

    def host_arrays(self):
        return list(self.inputs.values())

    def want(self):
        arrays = self._want()
        assert [(a.shape, a.dtype) for a in arrays] == [(tuple(s), np.dtype(d)) for _, s, d in self.outputs], self.name
        return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _rng(*key):
    return np.random.default_rng([20261021, *key])


def _frame(shape, dtype, *key):
    return _rng(*key).integers(0, int(np.iinfo(dtype).max) + 1, tuple(shape) + (3,)).astype(dtype)


def _doubles(values):
    v = np.asarray(values, np.float64).reshape(-1)
    return (C.c_double * v.size)(*v)


# ------------------------------------------------------------------------------------------------- the free functions
BLUR = (21, 50.0)       # BORDER_REPLICATE_BLUR with the pipeline's kernel


class WarpJob(FreeJob):
    """the blur's side buffer `tmp` is the job's own too, and is no output"""

    def prepare(self):
        super().prepare()
        self.ptr["tmp"] = self.empty(self.inputs["src"].nbytes).ptr


def warp_job(L, kind, shape, dtype, M, key):
    h, w = shape
    img = _frame(shape, dtype, 1, key)
    M = np.array(M, np.float64)
    m, bv = _doubles(M), _doubles(wc.border_value(dtype))

    def launch(j):
        lib = L.load()
        fn = lib.mi_warp_perspective_device if kind == "perspective" else lib.mi_warp_affine_device
        L.check(fn(0, j.stream, j.ptr["src"], j.ptr["dst"], j.ptr["tmp"], j.ptr["mask"], h, w, L.DTYPE_CODE[np.dtype(dtype)], m,
                   L.BORDER_REPLICATE_BLUR, bv, BLUR[0], BLUR[1]))

    return WarpJob(L, "warp %s" % kind, {"src": img}, [("dst", img.shape, dtype), ("mask", (h, w), np.uint8)], launch,
                   lambda: list(wc.oracle_warp(kind, img, M, 2, *BLUR)), dtype=dtype)


def unsharp_job(L, shape=(96, 160), dtype=np.uint8, args=(2.0, 1.5, 0.0)):
    import unsharp_restatement as usr
    from shinestacker_amd.sharpen import unsharp_mask_device
    h, w = shape
    img = _frame(shape, dtype, 2)
    return FreeJob(L, "unsharp mask", {"src": img}, [("dst", img.shape, dtype)],
                   lambda j: unsharp_mask_device(j.ptr["src"], j.ptr["dst"], h, w, dtype, *args, stream=j.stream),
                   lambda: [usr.unsharp_mask(img, *args)], dtype=dtype)


def nlm_job(L, shape=(96, 160), dtype=np.uint8, h_lum=3, template=7, search=21):
    import nlm_restatement as nlm
    from shinestacker_amd.denoise import weight_table
    from test_denoise_host import hash_noise
    h, w = shape
    y, x = np.mgrid[:h, :w]
    tex = np.rint(120 + 60 * np.sin(x / 37.0) * np.cos(y / 29.0)).astype(np.int64)
    img = np.clip(tex[:, :, None] + np.array([12, 0, -12]) + hash_noise((h, w, 3), 3, 6), 0, 255).astype(dtype)
    table, shift = weight_table(dtype, h_lum, template, search)

    def launch(j):
        L.check(L.load().mi_nlm_denoise_device(0, j.ptr["src"], j.ptr["dst"], h, w, L.DTYPE_CODE[np.dtype(dtype)], table.ctypes.data,
                                               int(table.size), int(shift), template, search, j.stream))

    return FreeJob(L, "NLM denoise", {"src": img}, [("dst", img.shape, dtype)], launch,
                   lambda: [nlm.denoise(img, h_lum, template, search)], dtype=dtype)


def stereo_job(L, shape=(120, 300), dtype=np.uint16, n_frames=9, shift=12.5, pivot=0.3, near="first"):
    import stereo_restatement as sr
    from shinestacker_amd.stereo import view_device
    h, w = shape
    img = _frame(shape, dtype, 4)
    depth = (_rng(4, 1).random(shape) * (n_frames - 1)).astype(np.float32)
    depth[:, w // 2:] = np.floor(depth[:, w // 2:])        # steps: holes and occlusions beside the smooth half
    return FreeJob(L, "stereo view", {"img": img, "depth": depth}, [("out", img.shape, dtype)],
                   lambda j: view_device(j.ptr["img"], j.ptr["depth"], j.ptr["out"], h, w, dtype, n_frames, shift, pivot, near,
                                         stream=j.stream),
                   lambda: [sr.view(img, depth, n_frames, shift, pivot, near)], dtype=dtype)


LENS = ((0.97, 0.02, 0, 0), (1, -0.12, 0.02, 0), (1.03, -0.01, 0, 0))       # barrel with lateral CA; B, G, R


def lens_job(L, shape=(200, 300), dtype=np.uint8):
    import lens_restatement as lr
    from shinestacker_amd.lens import Lens, correct_device
    h, w = shape
    img = _frame(shape, dtype, 5)
    return FreeJob(L, "lens remap", {"src": img}, [("dst", img.shape, dtype), ("mask", (h, w), np.uint8)],
                   lambda j: correct_device(j.ptr["src"], j.ptr["dst"], h, w, dtype, Lens(LENS), stream=j.stream,
                                            dev_mask=j.ptr["mask"]),
                   lambda: list(lr.remap(img, LENS, None, return_mask=True)), dtype=dtype)


def debayer_job(L, shape=(150, 262), dtype=np.uint16, pattern="GRBG"):
    import demosaic_restatement as dr
    from shinestacker_amd.demosaic import Cfa, debayer_device
    h, w = shape
    mosaic = _rng(6).integers(0, int(np.iinfo(dtype).max) + 1, shape).astype(dtype)
    return FreeJob(L, "debayer", {"mosaic": mosaic}, [("bgr", shape + (3,), dtype)],
                   lambda j: debayer_device(j.ptr["mosaic"], j.ptr["bgr"], h, w, dtype, Cfa(pattern), stream=j.stream),
                   lambda: [dr.demosaic(mosaic, pattern)], dtype=dtype)


def finish_job(L, shape=(131, 203), dtype=np.uint8, crop=(3, 5, 120, 190), orientation=6):
    import finish_restatement as fin
    h, w = shape
    img = _frame(shape, dtype, 7)
    out_shape = (crop[3], crop[2], 3) if orientation >= 5 else (crop[2], crop[3], 3)

    def launch(j):
        L.check(L.load().mi_frame_finish_device(0, j.stream, j.ptr["src"], j.ptr["dst"], h, w, L.DTYPE_CODE[np.dtype(dtype)], *crop,
                                                orientation))

    return FreeJob(L, "frame finish", {"src": img}, [("dst", out_shape, dtype)], launch,
                   lambda: [fin.finish(img, crop, orientation)], dtype=dtype)


def composite_job(L, shape=(100, 180), dtype=np.uint8, n=5):
    import depth_render_restatement as drr
    from shinestacker_amd.depth_render import composite_device
    h, w = shape
    frames = [_frame(shape, dtype, 8, i) for i in range(n)]
    depth = (_rng(8, 99).random(shape) * (n + 1) - 1).astype(np.float32)      # below 0 and above n - 1 too
    depth[0, 0], depth[::7, ::5] = np.nan, 2.0
    inputs = {"frame %d" % i: f for i, f in enumerate(frames)}
    inputs["depth"] = depth
    return FreeJob(L, "depth composite", inputs, [("out", frames[0].shape, dtype)],
                   lambda j: composite_device([j.ptr["frame %d" % i] for i in range(n)], 0, n, n, j.ptr["depth"], j.ptr["out"], h, w,
                                              dtype, "linear", stream=j.stream),
                   lambda: [drr.composite(frames, depth, "linear")], dtype=dtype)


def guided_job(L, shape=(96, 160), radius=6, eps=1e-4):
    import guided_cases as gc
    import guided_restatement as gr
    from shinestacker_amd import depth_out
    h, w = shape
    p, wt, g = gc.depth_plane(shape), gc.weight_plane(shape, np.float32, "random"), gc.guide_frame(shape, np.uint8, "random")
    lo, hi = float(p.min()), float(p.max())
    scratch = np.zeros(depth_out.SCRATCH_PLANES * h * w, np.float64)      # the job's own: the four launches are only queued
    return FreeJob(L, "guided refine", {"depth": p, "weight": wt, "guide": g, "scratch": scratch}, [("out", shape, np.float32)],
                   lambda j: depth_out.guided_refine_device(j.ptr["depth"], j.ptr["weight"], np.float32, j.ptr["guide"], np.uint8, h, w,
                                                            j.ptr["out"], lo, hi, radius, eps, scratch_ptr=j.ptr["scratch"],
                                                            stream=j.stream),
                   lambda: [gr.guided_refine(p, wt, g, radius, eps, lo, hi)], dtype=np.float32)


class ExtractJob(Job):
    """features.detect_and_compute: a host form, which uploads the frame, extracts on the null stream and downloads"""

    def __init__(self):
        super().__init__("feature detect_and_compute")
        import features_cases as fc
        self.frame = fc.scene_similarity()[4]

    def host_arrays(self):
        return [self.frame]

    def call(self, r):
        from shinestacker_amd import features as ft
        f = ft.detect_and_compute(self.frame)
        return f.kp.tobytes() + f.desc.tobytes()

    def want(self):
        import features_restatement as fr
        kp, desc = fr.extract(self.frame)
        assert len(kp) > 100
        return np.ascontiguousarray(kp, np.int32).tobytes() + np.ascontiguousarray(desc, np.uint8).tobytes()


class HistogramJob(DeviceJob):
    """mi_histogram_device: the counts come back to the host with the call"""

    def __init__(self, L, shape=(150, 200), dtype=np.uint16):
        super().__init__(L, "histogram")
        self.img, self.nbins, self.dtype = _frame(shape, dtype, 9), 65536 if dtype == np.uint16 else 256, np.int64

    def prepare(self):
        self.src, self.scratch = self.put(self.img), self.empty(3 * self.nbins * 4)

    def host_arrays(self):
        return [self.img]

    def call(self, r):
        counts = np.full((3, self.nbins), -1, np.int64)
        h, w = self.img.shape[:2]
        self.L.check(self.L.load().mi_histogram_device(0, None, self.src.ptr, self.scratch.ptr, h, w, self.L.DTYPE_CODE[self.img.dtype],
                                                       self.L.HIST_BGR, 1, 1, 0.0, counts.ctypes.data))
        return counts.tobytes()

    def want(self):
        return np.stack([np.bincount(self.img[..., c].ravel(), minlength=self.nbins) for c in range(3)]).astype(np.int64).tobytes()


def free_jobs_first(L):
    """6 device-form operations, each on its own buffers and the null stream"""
    h, w = 211, 333
    return [warp_job(L, "affine", (h, w), np.uint8, wc.about_centre(*wc.SIMILARITY[:2], h, w, *wc.SIMILARITY[2:]), 0),
            warp_job(L, "perspective", (130, 262), np.uint16, wc.MILD, 1),
            unsharp_job(L), nlm_job(L), stereo_job(L), lens_job(L)]


def free_jobs_second(L):
    return [debayer_job(L), finish_job(L), composite_job(L), guided_job(L), ExtractJob(), HistogramJob(L)]


# ------------------------------------------------------------------------------------------------------ the warp walks
LADDER = [(40, 70), (130, 262), (211, 333), (300, 500)]
WALKS = {       # (kind, dtype): the index into LADDER of every round
    ("perspective", np.uint8):  [0, 1, 1, 1, 1, 1, 1, 2, 2, 3, 3, 2, 1, 0, 0, 0, 0, 0, 0, 0],
    ("affine", np.uint8):       [0, 0, 1, 2, 2, 2, 2, 2, 3, 3, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0],
    ("perspective", np.uint16): [0, 0, 0, 0, 1, 2, 3, 3, 3, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    ("affine", np.uint16):      [0, 0, 0, 0, 0, 1, 2, 3, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
}


def scratch_requests(kind, shape):
    """what a warp with the border blur asks of the two caches: (tiles in the blur's list, ints in the coordinate tables)"""
    h, w = shape
    k = wc.CONSTANTS
    return -(-h // k["BT_H"]) * -(-w // k["BT_W"]), 2 * (w + h) if kind == "affine" else 0


def walk_matrix(kind, shape):
    return np.array(wc.MILD if kind == "perspective" else wc.about_centre(*wc.SIMILARITY[:2], *shape, *wc.SIMILARITY[2:]), np.float64)


class WarpWalk(DeviceJob):
    """round r warps the frame of size LADDER[walk[r]]: one source per size, one destination, side buffer and mask of the
    largest size.  A call returns the warped frame and its valid mask."""

    def __init__(self, L, kind, dtype, walk, own_stream=False):
        super().__init__(L, "%s %s" % (kind, np.dtype(dtype).name), own_stream)
        self.kind, self.dtype, self.walk = kind, dtype, list(walk)
        self.frames = {i: _frame(LADDER[i], dtype, 10, i, np.dtype(dtype).itemsize, kind == "affine") for i in sorted(set(walk))}

    def prepare(self):
        self.open_stream()
        big = max(f.nbytes for f in self.frames.values())
        self.src = {i: self.put(f) for i, f in self.frames.items()}
        self.dst, self.tmp = self.put(np.full(big, 0xA5, np.uint8)), self.empty(big)
        self.mask = self.put(np.full(big // (3 * np.dtype(self.dtype).itemsize), 0xEE, np.uint8))

    def call(self, r):
        L, i = self.L, self.walk[r]
        h, w = LADDER[i]
        lib = L.load()
        fn = lib.mi_warp_perspective_device if self.kind == "perspective" else lib.mi_warp_affine_device
        L.check(fn(0, self.stream, self.src[i].ptr, self.dst.ptr, self.tmp.ptr, self.mask.ptr, h, w, L.DTYPE_CODE[np.dtype(self.dtype)],
                   _doubles(walk_matrix(self.kind, (h, w))), L.BORDER_REPLICATE_BLUR, _doubles(wc.border_value(self.dtype)), *BLUR))
        self.wait()
        return self.dst.download((h, w, 3), self.dtype).tobytes() + self.mask.download((h, w), np.uint8).tobytes()

    def want(self):
        out = {}
        for i, f in self.frames.items():
            img, mask = wc.oracle_warp(self.kind, f, walk_matrix(self.kind, LADDER[i]), 2, *BLUR)
            assert 0 < int((mask == 0).sum()) < mask.size, "the blur needs masked pixels, and others"
            out[i] = img.tobytes() + mask.tobytes()
        return out

    def expected_at(self, r):
        return self.expected[self.walk[r]]

    def host_arrays(self):
        return list(self.frames.values())

    def differing(self, got, r):
        h, w = LADDER[self.walk[r]]
        n = h * w * 3 * np.dtype(self.dtype).itemsize
        want = self.expected_at(r)
        return differing_elements(got[:n], want[:n], self.dtype) + differing_elements(got[n:], want[n:])


def warp_walk_jobs(L, own_stream=False):
    return [WarpWalk(L, kind, dtype, walk, own_stream) for (kind, dtype), walk in WALKS.items()]


# ------------------------------------------------------------------------------------------------------------ handles
class HandleJob(Job):
    """one handle: create() (prepare), feed() then finish() -> bytes (a call), close() (release).  The three phases are
    what test e runs on three threads."""

    def __init__(self, L, name):
        super().__init__(name)
        self.L, self.h, self.bufs = L, None, []

    def prepare(self):
        self.create()

    def call(self, r):
        self.feed()
        return self.finish()

    def release(self):
        self.close()

    def close(self):
        if self.h is not None:
            self.h.close()
            self.h = None
        for b in self.bufs:
            b.free()
        self.bufs = []

    def upload(self, frames):
        """the frames side by side in one device buffer: their addresses"""
        nb = frames[0].nbytes
        buf = self.L.DeviceBuffer(nb * len(frames))
        self.bufs.append(buf)
        for i, f in enumerate(frames):
            buf.upload(np.ascontiguousarray(f), i * nb)
        return [buf.ptr + i * nb for i in range(len(frames))]

    def buffers(self):
        return [(b.ptr, b.nbytes) for b in self.bufs]

    def host_arrays(self):
        return list(getattr(self, "frames", [])) + [a for a in (getattr(self, "ref", None), getattr(self, "mov", None)) if a is not None]


class StackJob(HandleJob):
    """a Stack fed from host arrays: reset, push every frame, finish; against oracle.StreamingOracle, byte for byte"""

    def __init__(self, L, oracle, name, shape, dtype, n, arith, min_size, key):
        super().__init__(L, name)
        self.oracle, self.shape, self.in_dtype, self.arith, self.min_size = oracle, shape, np.dtype(dtype), arith, min_size
        self.out_dtype = np.dtype(np.uint8 if self.in_dtype == np.float32 else dtype)
        hi = int(np.iinfo(self.out_dtype).max) + 1
        self.frames = [_rng(11, key, i).integers(0, hi, shape + (3,)).astype(dtype) for i in range(n)]
        self.frames[-1][:shape[0] // 2] = self.frames[0][:shape[0] // 2]       # exact ties: the first maximum must win
        self.dtype = self.out_dtype

    def create(self):
        self.h = self.L.Stack(*self.shape, in_dtype=self.in_dtype, out_dtype=self.out_dtype, arith=self.arith, min_size=self.min_size)

    def feed(self):
        self.h.reset()
        for f in self.frames:
            self.h.push_frame(f)

    def finish(self):
        return self.h.finish().tobytes()

    def want(self):
        so = self.oracle.StreamingOracle(*self.shape, self.out_dtype, arith=self.arith, min_size=self.min_size, keep_gauss=False)
        assert so.levels >= 2
        for f in self.frames:
            so.push_frame(f)
        out = so.finish()
        assert out.dtype == self.out_dtype
        return out.tobytes()


class DepthMapJob(HandleJob):
    """a DepthMap: reset, push, finish; against oracle/depth_map_oracle.py by the rule of test_gpu_depth_map.py (at most one
    count on at most 0.1 % of the values)"""

    def __init__(self, L, shape=(96, 160), dtype=np.uint8, n=3):
        super().__init__(L, "DepthMap")
        from test_gpu_depth_map import scene
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.frames = scene(_rng(12), n, *shape, dtype)

    def create(self):
        self.h = self.L.DepthMap(*self.shape, dtype=self.dtype)

    def feed(self):
        self.h.reset()
        for f in self.frames:
            self.h.push_frame(f)

    def finish(self):
        return self.h.finish().tobytes()

    def want(self):
        from oracle import depth_map_oracle as dmo
        out = dmo.depth_map_stack(self.frames)
        assert out.dtype == self.dtype
        return out.tobytes()

    def differing(self, got, r):
        want = self.expected
        if len(got) != len(want):
            return max(len(got), len(want))
        d = np.abs(np.frombuffer(got, self.dtype).astype(np.int64) - np.frombuffer(want, self.dtype).astype(np.int64))
        return 0 if d.max() <= 1 and (d != 0).mean() <= 1e-3 else int((d != 0).sum())


ECC_CASE = (387, 509, np.uint8, 2, (-0.8, 0.994, -12.4, 9.7), 60)    # of test_gpu_ecc_oracle.py's converged cases: a 194 x 255 grid
ECC_TOL_PX, ECC_TOL_RHO = 2e-3, 1e-5                                  # that file's tol_converged and TOL_RHO


class AlignerJob(HandleJob):
    """an Aligner: set_reference, estimate_batch of one moving frame; against oracle/ecc_oracle.py as
    test_gpu_ecc_oracle.py::test_converged_estimate holds it: the corners within ECC_TOL_PX, rho within ECC_TOL_RHO, the
    iterations within one per level"""

    def __init__(self, L, oracle):
        super().__init__(L, "Aligner")
        from ecc_pairs import make_pair, similarity
        h, w, dtype, self.s, motion, self.iters = ECC_CASE
        self.shape, self.dtype_in = (h, w), dtype
        self.ref, self.mov = make_pair(oracle, similarity(*motion, (w - 1) / 2, (h - 1) / 2), h=h, w=w, noise=5.0, seed=0, dtype=dtype)
        self.dtype = np.float64

    def create(self):
        self.ptrs = self.upload([self.ref, self.mov])
        self.h = self.L.Aligner(*self.shape, self.dtype_in, subsample=self.s, fast=True)

    def feed(self):
        self.h.set_reference(self.ptrs[0])

    def finish(self):
        m, cc, it = self.h.estimate_batch(self.ptrs[1:], max_iters=self.iters)
        return np.concatenate([m[0].reshape(-1), cc[:1], it[:1].astype(np.float64)]).tobytes()

    def want(self):
        from oracle import ecc_oracle as eo
        r = eo.solve_pyramids(eo.frame_pyramid(self.ref, self.s, False, 0), eo.frame_pyramid(self.mov, self.s, False, 0), s=self.s,
                              max_iters=self.iters)
        self.levels = len(r.level_iters)
        return np.concatenate([np.asarray(r.M, np.float64).reshape(-1)[:6], [r.cc, float(r.iters)]]).tobytes()

    def differing(self, got, r):
        from oracle import ecc_oracle as eo
        g, w = np.frombuffer(got, np.float64), np.frombuffer(self.expected, np.float64)
        if g.size != 8:
            return 8
        bad = not eo.corner_deviation(g[:6].reshape(2, 3), w[:6].reshape(2, 3), *self.shape) < ECC_TOL_PX
        return int(bad) + int(not abs(g[6] - w[6]) < ECC_TOL_RHO) + int(not abs(g[7] - w[7]) <= self.levels)


class FeatureAlignerJob(HandleJob):
    """a FeatureAligner on features_cases.scene_similarity(): set_reference, estimate_batch; the good matches equal
    features_restatement's, the transform within rtol 1e-9 (atol 1e-12) of its refit, as test_gpu_feature_aligner.py holds it"""
    K = 300

    def __init__(self, L, make=None):
        super().__init__(L, "FeatureAligner")
        import features_cases as fc
        self.make = make
        self.height, self.width, _, self.mov, self.ref = fc.scene_similarity()
        self.cfgs = ({"match_method": "KNN", "threshold": 0.75}, {"transform": "ALIGN_RIGID", "rans_threshold": 3.0, "max_iters": self.K})
        self.dtype = np.float64

    def create(self):
        from shinestacker_amd import features as ft
        self.ptrs = self.upload([self.ref, self.mov])
        self.h = (self.make or ft.FeatureAligner)(self.height, self.width, self.ref.dtype, ft.FeatureParams(), max_batch=1)

    def feed(self):
        self.h.set_reference(self.ptrs[0])

    def finish(self):
        (n_good, m, frac), = self.h.estimate_batch(self.ptrs[1:], *self.cfgs)
        assert m is not None and m.shape == (2, 3) and 0.0 < frac <= 1.0
        return np.concatenate([[float(n_good)], np.asarray(m, np.float64).reshape(-1)]).tobytes()

    def want(self):
        import feature_aligner_cases as ac
        import features_restatement as fr
        w = ac.expected_pair(self.mov, self.ref, 3, 2000, 20, "KNN", 0.75, fr.SIMILARITY, 3.0, self.K, 0)
        assert len(w["good"]) >= 100 and w["m"] is not None
        return np.concatenate([[float(len(w["good"]))], np.asarray(w["m"], np.float64).reshape(-1)[:6]]).tobytes()

    def differing(self, got, r):
        g, w = np.frombuffer(got, np.float64), np.frombuffer(self.expected, np.float64)
        if g.size != 7:
            return 7
        return int(g[0] != w[0]) + int((~np.isclose(g[1:], w[1:], rtol=1e-9, atol=1e-12)).sum())


def handle_jobs(L, oracle, feature_aligner=None):
    """one handle per thread: 6 jobs"""
    return [StackJob(L, oracle, "Stack separable uint8", (133, 201), np.uint8, 4, "separable", 8, 0),
            StackJob(L, oracle, "Stack exact uint16", (96, 160), np.uint16, 3, "exact", 16, 1),
            StackJob(L, oracle, "Stack separable float32", (150, 226), np.float32, 3, "separable", 8, 2),
            DepthMapJob(L), AlignerJob(L, oracle), FeatureAlignerJob(L, feature_aligner)]


class Phases:
    """what run_phases saw: the result of finish(), or the exception with the phase it was raised in, or the phase that had
    not returned at the deadline"""

    def __init__(self):
        self.result, self.error, self.alive, self.threads = None, None, None, []


def run_phases(job, deadline_s=DEADLINE_S):
    """A handle that changes threads: create() on thread A, feed() on thread B, finish() and close() on thread C; each is
    joined before the next starts.  Nothing of the handle is freed here if a thread does not return."""
    out = Phases()
    t_end = time.monotonic() + deadline_s

    def finish_and_close():
        try:
            out.result = job.finish()
        finally:
            job.close()

    for name, fn in (("create", job.create), ("feed", job.feed), ("finish and close", finish_and_close)):
        def work(fn=fn, name=name):
            out.threads.append(threading.current_thread())      # (the objects: an ended thread's ident is handed out again)
            try:
                fn()
            except BaseException as e:  # noqa: BLE001  (reported: the caller asserts error is None)
                out.error = (name, e)
        t = threading.Thread(target=work, name="%s: %s" % (job.name, name), daemon=True)
        t.start()
        t.join(max(0.0, t_end - time.monotonic()))
        if t.is_alive():
            out.alive = name
            return out
        if out.error:
            if name != "finish and close":
                closer = threading.Thread(target=job.close, daemon=True)
                closer.start()
                closer.join(max(0.0, t_end - time.monotonic()))
            return out
    return out


# ------------------------------------------------------------------------------------------------------ mi_last_error
INVALID_CALLS = [       # (name, what replaces the good arguments, the text test_gpu_feature_aligner.py expects)
    ("null frame list", {"movs": None}, "null frame list"),
    ("max_iters 0", {"k": 0}, "max_iters must be in [1, 4096]"),
    ("unknown kind", {"kind": 2}, "unknown kind 2"),
    ("ratio NaN", {"ratio": float("nan")}, "ratio must be finite"),
]
ERROR_ROUNDS = 50


class InvalidCallJob(HandleJob):
    """one invalid mi_feat_aligner_estimate_batch on a handle of the job's own: the status, and which of the four messages
    mi_last_error then holds on this thread"""

    def __init__(self, L, name, change, text, make=None):
        super().__init__(L, name)
        self.change, self.text, self.make = change, text, make

    def create(self):
        from shinestacker_amd import features as ft
        self.frame = self.upload([np.zeros((96, 160, 3), np.uint8)])[0]
        self.h = (self.make or ft.FeatureAligner)(96, 160, np.uint8, ft.FeatureParams(1, 64, 20), max_batch=1)
        cap = self.h._al.max_matches
        self.out = np.zeros(cap * 16, np.uint8)
        o = self.out.ctypes.data
        good = dict(movs=(C.c_void_p * 1)(self.frame), n=1, method=0, ratio=0.75, kind=0, thr=3.0, k=100, seed=0, cap=cap, n_good=o,
                    winner=o, models=o, inliers=o, mask=o, src=o, dst=o)
        self.args = list({**good, **self.change}.values())

    def call(self, r):
        L = self.L
        rc = L.load().mi_feat_aligner_estimate_batch(self.h._al._h, *self.args)
        msg = L.last_error()
        return ("%d: %s" % (rc, ", ".join(t for _, _, t in INVALID_CALLS if t in msg))).encode()

    def want(self):
        return ("%d: %s" % (self.L.MI_ERR_INVALID, self.text)).encode()


class NoErrorJob(Job):
    """a thread that makes no failing call reads the empty message.  (On the main thread, where run_jobs calls every job
    once, only the call is made: earlier tests of the same process have failed calls there on purpose.)"""

    def __init__(self, L):
        super().__init__("no failing call")
        self.L = L

    def call(self, r):
        n = self.L.device_count()
        msg = "" if threading.current_thread() is threading.main_thread() else self.L.last_error()
        return ("%d: %s" % (min(n, 1), msg)).encode()

    def want(self):
        return b"1: "


def error_jobs(L, feature_aligner=None):
    return [InvalidCallJob(L, name, change, text, feature_aligner) for name, change, text in INVALID_CALLS] + [NoErrorJob(L)]


# ------------------------------------------------------------------------------------------- free functions beside handles
def mixed_jobs(L, oracle, feature_aligner=None):
    """the 6 free-function jobs of free_jobs_first on the null stream beside three handles on their own non-blocking streams.
    Nine jobs on MAX_THREADS = 8 threads: the two smallest free functions share a thread, one after the other."""
    free = free_jobs_first(L)
    by_name = {j.name: j for j in free}
    pair = Sequence(by_name.pop("unsharp mask"), by_name.pop("NLM denoise"))
    handles = [j for j in handle_jobs(L, oracle, feature_aligner) if j.name in ("Stack separable uint8", "DepthMap", "Aligner")]
    return list(by_name.values()) + [pair] + handles


TABLES = {      # test of test_gpu_threads.py -> its jobs
    "a, first": lambda L, oracle, fa=None: free_jobs_first(L),
    "a, second": lambda L, oracle, fa=None: free_jobs_second(L),
    "b": lambda L, oracle, fa=None: warp_walk_jobs(L),
    "c": lambda L, oracle, fa=None: warp_walk_jobs(L, own_stream=True),
    "d": handle_jobs,
    "f": lambda L, oracle, fa=None: error_jobs(L, fa),
    "g": mixed_jobs,
}
