"""CPU: the runner of tests/thread_cases.py reports what it is there to report -- with pure-Python jobs: jobs that share nothing
pass, a race on an unlocked counter is a mismatch with the job's name and the round, an exception is reported as it was
raised, a job that blocks is reported alive at the deadline instead of hanging the test -- and the job tables of
test_gpu_threads.py mean something: the warp walks grow and shrink, each thread is somewhere the first to ask a cache for
more, no two jobs of a test own the same buffer, no test has more than 8 threads."""
import itertools
import threading
import time

import numpy as np
import pytest

import thread_cases as tc


def constant(name, value=b"\x01\x02\x03\x04"):
    return tc.FnJob(name, lambda r: value, value)


# ---------------------------------------------------------------------------------------------------------------- runner
def test_jobs_that_share_nothing_pass():
    state = {n: [] for n in "abcd"}

    def job(n):
        def call(r):
            state[n].append(r)
            return bytes([r % 256]) * 8
        j = tc.FnJob(n, call, None)
        j.expected_at = lambda r: bytes([r % 256]) * 8
        return j

    report = tc.run_threads([job(n) for n in "abcd"], 20, 10.0)
    assert report.ok and str(report).startswith("ok"), str(report)
    assert report.calls == {n: 20 for n in "abcd"} and all(state[n] == list(range(20)) for n in "abcd")
    assert report.mismatches == [] and report.errors == [] and report.alive == []


def test_a_race_on_an_unlocked_counter_is_a_mismatch_with_name_and_round():
    """Two jobs add 1 to one counter without a lock: read, time.sleep(0), write.  A job answers whether anybody wrote between
    its read and its write, and keeps its own list of the rounds where somebody did.  Whether the two meet by themselves is
    the scheduler's business, so in round 7 they are made to: the second job reads only after the first has read, and the
    first writes only after the second has written -- the first job's update of round 7 is the lost one.  The runner must
    report that round under that name, and beyond it exactly the rounds the jobs saw themselves."""
    shared, seen = [0], []
    first_read, second_wrote = threading.Event(), threading.Event()

    def add_one(name, r, after_read=None):
        v = shared[0]
        if after_read:
            after_read()
        time.sleep(0)
        clean = shared[0] == v
        shared[0] = v + 1
        if not clean:
            seen.append((name, r))
        return b"clean" if clean else b"raced"

    def first(r):
        return add_one("first", r, (lambda: (first_read.set(), second_wrote.wait(10.0))) if r == 7 else None)

    def second(r):
        if r == 7:
            first_read.wait(10.0)
        out = add_one("second", r)
        if r == 7:
            second_wrote.set()
        return out

    rounds = 50
    report = tc.run_threads([tc.FnJob("first", first, b"clean"), tc.FnJob("second", second, b"clean")], rounds, 30.0)
    assert ("first", 7) in seen and ("first", 7, 5) in report.mismatches
    assert not report.errors and not report.alive and not report.ok
    assert sorted(report.mismatches) == sorted((n, r, 5) for n, r in seen)
    assert report.calls == {"first": rounds, "second": rounds}       # a mismatch does not end a thread
    assert "first, round 7: 5 differ" in str(report) or len(report.mismatches) > 12
    assert shared[0] < 2 * rounds                                    # an update was lost


def test_a_job_that_raises_is_reported_with_its_exception():
    boom = ValueError("boom")

    def call(r):
        if r == 3:
            raise boom
        return b"ok"

    report = tc.run_threads([tc.FnJob("raises", call, b"ok"), constant("other")], 20, 10.0)
    assert report.errors == [("raises", 3, boom)] and report.calls["raises"] == 3
    assert not report.ok and not report.alive and not report.mismatches
    assert "raises, round 3: ValueError('boom')" in str(report)
    assert report.calls["other"] <= 20          # the flag stops the others before their next call


def test_a_job_that_blocks_is_reported_alive_at_the_deadline():
    gate, entered = threading.Event(), threading.Event()

    def blocks(r):
        entered.set()
        return gate.wait(30.0) and b"late"

    def returns(r):
        entered.wait(10.0)
        return b"here"

    try:
        t0 = time.monotonic()
        report = tc.run_threads([tc.FnJob("blocks", blocks, b"late"), tc.FnJob("returns", returns, b"here")], 5, 1.0)
        took = time.monotonic() - t0
        assert report.alive == ["blocks"] and "alive: [blocks]" in str(report) and not report.ok
        assert 1.0 <= took < 2.0, took
        assert report.calls == {"blocks": 0, "returns": 5}
        assert report.overlapped == {"blocks": 1, "returns": 5}         # every call of one ran inside the other's only call
    finally:
        gate.set()


def test_run_jobs_checks_every_job_alone_first_and_frees_nothing_under_a_live_thread():
    log = []
    wrong = tc.FnJob("wrong", lambda r: b"\x00\x01", b"\x00\x02", lambda: log.append("prepare"), lambda: log.append("release"))
    with pytest.raises(AssertionError, match="on the main thread"):
        tc.run_jobs([wrong, constant("fine")], 3, 5.0)
    assert log == ["prepare", "release"]
    gate, log = threading.Event(), []
    try:
        first = []

        def call(r):
            if first:
                gate.wait(30.0)
            first.append(r)
            return b"x"

        report = tc.run_jobs([tc.FnJob("blocks", call, b"x", None, lambda: log.append("release"))], 3, 0.5)
        assert report.alive == ["blocks"] and log == []
    finally:
        gate.set()
    with pytest.raises(AssertionError):
        tc.run_jobs([constant("job %d" % i) for i in range(tc.MAX_THREADS + 1)], 1, 5.0)


def test_differing_elements_and_shared_buffers():
    a = np.arange(8, dtype=np.uint16)
    b = a.copy()
    b[[2, 5]] += 256
    assert tc.differing_elements(a.tobytes(), a.tobytes(), np.uint16) == 0
    assert tc.differing_elements(a.tobytes(), b.tobytes(), np.uint16) == 2 == tc.differing_elements(a.tobytes(), b.tobytes())
    assert tc.differing_elements(a.tobytes(), a.tobytes()[:-1]) == 16
    nan = np.array([np.nan, 1.0], np.float32)
    assert tc.differing_elements(nan.tobytes(), nan.tobytes(), np.float32) == 0

    def owner(name, spans):
        j = constant(name)
        j.buffers = lambda: spans
        return j

    assert tc.shared_buffers([owner("a", [(100, 50), (400, 8)]), owner("b", [(150, 10)]), owner("c", [(160, 240)])]) == []
    assert tc.shared_buffers([owner("a", [(100, 50)]), owner("b", [(149, 1)])]) == [("a", "b")]
    three = [owner("a", [(100, 500)]), owner("b", [(10, 10), (200, 4)]), owner("c", [(599, 2)])]
    assert tc.shared_buffers(three) == [("a", "b"), ("a", "c")]
    seq = tc.Sequence(owner("a", [(0, 4)]), owner("b", [(2, 4)]))
    assert seq.buffers() == [(0, 4), (2, 4)] and seq.name == "a + b"
    assert seq.differing(seq.call(0), 0) == 0 and seq.differing((b"\x01\x02\x03\x05", b"\x01\x02\x03\x04"), 0) == 1


# ---------------------------------------------------------------------------------------------------------------- tables
def test_every_walk_grows_then_shrinks_over_the_whole_ladder():
    assert tc.LADDER == [(40, 70), (130, 262), (211, 333), (300, 500)]
    assert set(tc.WALKS) == {(k, d) for k in ("affine", "perspective") for d in (np.uint8, np.uint16)}
    sizes = [tc.scratch_requests("affine", s) for s in tc.LADDER]
    assert [t for t, _ in sizes] == [-(-h // 32) * -(-w // 64) for h, w in tc.LADDER] == [4, 25, 42, 80]
    assert [c for _, c in sizes] == [2 * (h + w) for h, w in tc.LADDER] and tc.scratch_requests("perspective", (300, 500)) == (80, 0)
    assert sizes == sorted(sizes) and len(set(sizes)) == 4        # up the ladder both requests grow
    peaks = []
    for key, walk in tc.WALKS.items():
        assert len(walk) == tc.ROUNDS and walk[0] == 0 == walk[-1] and set(walk) == {0, 1, 2, 3}, key
        top = walk.index(3)
        assert walk[:top + 1] == sorted(walk[:top + 1]) and walk[top:] == sorted(walk[top:], reverse=True), key
        assert all(abs(a - b) <= 1 for a, b in zip(walk, walk[1:])), key        # every size on the way up and on the way down
        peaks.append(top)
    assert len(set(peaks)) == len(peaks)        # the largest frames come at different rounds


def test_every_thread_is_somewhere_the_first_to_ask_a_cache_for_more():
    """with the threads in step: at some round r >= 1 the thread asks the tile list or the coordinate tables for more than
    every thread has asked in the rounds before r, so that the cache all four share is re-allocated by this thread while the
    others, which have called before, may have work queued on it"""
    first = {key: [] for key in tc.WALKS}
    for cache in (0, 1):
        for key, walk in tc.WALKS.items():
            for r in range(1, tc.ROUNDS):
                mine = tc.scratch_requests(key[0], tc.LADDER[walk[r]])[cache]
                before = [tc.scratch_requests(k[0], tc.LADDER[w[q]])[cache] for k, w in tc.WALKS.items() for q in range(r)]
                same_round = [tc.scratch_requests(k[0], tc.LADDER[w[r]])[cache] for k, w in tc.WALKS.items() if k != key]
                if mine > max(before) and mine > max(same_round):
                    first[key].append((("tiles", "coordinates")[cache], r))
    assert all(first.values()), first
    grown = sorted(r for v in first.values() for _, r in v)
    assert len(set(grown)) >= 4      # and not all in one round


class FakeBuffer:
    """DeviceBuffer without a device: addresses from a counter, 256-byte aligned as the allocator's"""
    next_address = itertools.count(1 << 20, 1 << 24)

    def __init__(self, nbytes, device=0):
        assert nbytes < 1 << 24
        self.ptr, self.nbytes = next(FakeBuffer.next_address), int(nbytes)

    def upload(self, arr, offset=0):
        assert offset + np.ascontiguousarray(arr).nbytes <= self.nbytes

    def free(self):
        self.ptr = None


class FakeHandle:
    streams = itertools.count(7)

    def __init__(self, *a, **kw):
        self.stream = next(FakeHandle.streams)
        self._al = self
        self.max_matches = 64

    def close(self):
        pass


class FakeLib:
    DeviceBuffer, Stack, DepthMap, Aligner = FakeBuffer, FakeHandle, FakeHandle, FakeHandle


@pytest.mark.parametrize("test", list(tc.TABLES))
def test_no_two_jobs_of_a_test_share_a_buffer_and_no_test_has_more_than_8_threads(oracle, test):
    jobs = tc.TABLES[test](FakeLib, oracle, FakeHandle)
    assert 4 <= len(jobs) <= tc.MAX_THREADS == 8
    assert len({j.name for j in jobs}) == len(jobs)
    try:
        for j in jobs:
            j.prepare()
        assert all(j.buffers() or j.host_arrays() or j.name == "no failing call" for j in jobs)
        assert tc.shared_buffers(jobs) == []
        arrays = [a for j in jobs for a in j.host_arrays()]
        assert all(isinstance(a, np.ndarray) for a in arrays)
        assert len({id(a) for a in arrays}) == len(arrays)       # nor a host array they upload
        if test == "c":
            assert len({j.stream for j in jobs}) == len(jobs) and None not in {j.stream for j in jobs}
        if test in ("a, first", "a, second", "b"):
            assert {getattr(j, "stream", None) for j in jobs} == {None}
    finally:
        for j in jobs:
            j.release()


def test_the_tables_are_the_ones_the_issue_names(oracle):
    names = {t: [j.name for j in tc.TABLES[t](FakeLib, oracle, FakeHandle)] for t in tc.TABLES}
    assert names["a, first"] == ["warp affine", "warp perspective", "unsharp mask", "NLM denoise", "stereo view", "lens remap"]
    assert names["a, second"] == ["debayer", "frame finish", "depth composite", "guided refine", "feature detect_and_compute", "histogram"]
    assert names["b"] == names["c"] == ["perspective uint8", "affine uint8", "perspective uint16", "affine uint16"]
    assert names["d"] == ["Stack separable uint8", "Stack exact uint16", "Stack separable float32", "DepthMap", "Aligner", "FeatureAligner"]
    assert names["f"] == ["null frame list", "max_iters 0", "unknown kind", "ratio NaN", "no failing call"]
    assert names["g"] == ["warp affine", "warp perspective", "stereo view", "lens remap", "unsharp mask + NLM denoise",
                          "Stack separable uint8", "DepthMap", "Aligner"]
    assert tc.ROUNDS == 20 and tc.DEADLINE_S == 60.0 and tc.ERROR_ROUNDS == 50
