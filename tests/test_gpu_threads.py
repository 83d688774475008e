"""GPU: the library called from several threads at once equals its restatements.

INTEGRATION.md promises "one thread per handle at a time; any thread", the pipeline and the GUI rely on it, and the library
holds state that only threads reach: the warp's two scratch caches and its enqueue locks, keyed by (device, stream); the
thread-local guards around hipFuncSetAttribute; the thread-local text of mi_last_error; hipSetDevice in every entry point;
the pinned-copy pool.  Every test here runs the jobs of tests/thread_cases.py -- at most 8 threads, released together, 20
rounds each, one 60 s deadline -- and every result of every round must equal what the NumPy restatements and the oracle say,
computed before any thread starts; each job has equalled it once on the main thread by then, so a difference is the
threads'.  test_thread_cases_host.py shows on the CPU that the runner reports a race, an exception and a thread that does
not return.  A run that reaches the deadline is a hang: the test fails, nothing is freed under the thread and nothing is
tried again.

  b  warps that grow the null stream's scratch under each other    (first in the file: the cache only grows)
  a  free functions on the null stream, 6 + 6 operations
  c  the warps of b on the threads' own streams
  d  one handle per thread
  e  a handle made on one thread, fed on a second, finished and closed on a third
  f  mi_last_error is per thread
  g  free functions on the null stream beside handles on their non-blocking streams"""
import threading

import pytest

import thread_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hiplib):
    hiplib.require_device()
    return hiplib


def passed(report, jobs, rounds=tc.ROUNDS):
    print(report)
    assert report.ok, str(report)
    assert report.calls == {j.name: rounds for j in jobs}


def test_b_warps_grow_the_shared_scratch_under_each_other(L, oracle):
    jobs = tc.warp_walk_jobs(L)
    assert len(jobs) == 4
    passed(tc.run_jobs(jobs), jobs)


def test_a_free_functions_on_the_null_stream(L, oracle):
    jobs = tc.free_jobs_first(L)
    assert len(jobs) == 6
    passed(tc.run_jobs(jobs), jobs)


def test_a_six_more_free_functions_on_the_null_stream(L, oracle):
    jobs = tc.free_jobs_second(L)
    assert len(jobs) == 6
    passed(tc.run_jobs(jobs), jobs)


def test_c_warps_on_the_threads_own_streams(L, oracle):
    jobs = tc.warp_walk_jobs(L, own_stream=True)
    report = tc.run_jobs(jobs)
    passed(report, jobs)


def test_d_one_handle_per_thread(L, oracle):
    jobs = tc.handle_jobs(L, oracle)
    assert len(jobs) == 6
    passed(tc.run_jobs(jobs), jobs)


def test_e_a_handle_that_changes_threads(L, oracle):
    """create, feed, finish + close on three threads, none of which has called the library before: hipSetDevice and the
    thread-local attribute guards on a thread the handle was not made on"""
    jobs = {j.name: j for j in tc.handle_jobs(L, oracle)}
    for name in ("Stack separable uint8", "DepthMap", "Aligner", "FeatureAligner"):
        job = jobs[name]
        job.expected
        out = tc.run_phases(job)
        assert out.alive is None, (name, "did not return from", out.alive)
        assert out.error is None, (name, out.error)
        assert len(set(out.threads)) == 3 and threading.main_thread() not in out.threads
        assert job.differing(out.result, 0) == 0, (name, job.differing(out.result, 0))


def test_f_last_error_is_per_thread(L):
    jobs = tc.error_jobs(L)
    assert len(jobs) == 5
    passed(tc.run_jobs(jobs, rounds=tc.ERROR_ROUNDS), jobs, tc.ERROR_ROUNDS)


def test_g_free_functions_beside_handles(L, oracle):
    jobs = tc.mixed_jobs(L, oracle)
    assert len(jobs) == tc.MAX_THREADS
    passed(tc.run_jobs(jobs), jobs)
