"""CPU: csrc/host_copy.hpp -- the banded bounce copy every host push goes through (copy_rows on the CopyPool) -- compiled for
the host into tools/host_copy_check.cpp and run as a child process: the copy equals a plain row loop for rows 1, 3, 4, 5 and 7
with 1 and 4 threads (bands are empty when there are fewer rows than threads), row bytes 1, 13 and 4096, a source stride equal
to the row and 5 bytes wider, one-row spans of 1, 3 and 1000 bytes, and two caller threads using the pool at once; guard bytes
around the destination stay untouched.  One build carries the address and undefined-behaviour sanitizers, linked statically,
so the program does not care what else the process loads; where the compiler links it, a second carries the thread sanitizer.
Where no compiler links the first pair the program is built plain."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "host_copy_check.cpp")
CASES = 5 * 3 * 2 * 2 + 3 * 2 + 200


def _compilers():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        path = shutil.which(name) if name else None
        if path:
            yield path


def _build(exe, flag_sets):
    """the first of `flag_sets` that some compiler builds: (its flags, None), or (None, the last failure)"""
    tried = None
    for flags in flag_sets:
        for cxx in _compilers():
            # (g++ links the runtimes dynamically unless told otherwise; clang links them statically and does not know the g++ flags)
            if flags and ("clang" in os.path.basename(os.path.realpath(cxx))) != ("-static-libsan" in flags):
                continue
            cmd = [cxx, "-std=c++17", "-O1", "-g", "-pthread", *flags, SOURCE, "-o", exe]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode == 0:
                return flags, None
            tried = (cmd, res.stderr[-2000:])
    return None, tried


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stderr == "", res.stderr[-3000:]
    assert res.stdout.split() == ["ok", str(CASES)]


def test_copy_rows_equals_the_row_loop_under_asan_and_ubsan(tmp_path):
    if not list(_compilers()):
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "host_copy_check")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    flags, failure = _build(exe, (sanitize + ["-static-libasan", "-static-libubsan"], sanitize + ["-static-libsan"], []))
    assert flags is not None, f"tools/host_copy_check.cpp does not compile: {failure}"
    _run(exe)


def test_copy_pool_is_race_free_under_tsan(tmp_path):
    exe = str(tmp_path / "host_copy_check_tsan")
    sanitize = ["-fsanitize=thread", "-fno-sanitize-recover=all"]
    flags, _ = _build(exe, (sanitize + ["-static-libtsan"], sanitize + ["-static-libsan"]))
    if flags is None:
        pytest.skip("no compiler on this machine links the thread sanitizer")
    _run(exe)
