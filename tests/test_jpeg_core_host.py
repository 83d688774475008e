"""CPU: csrc/jpeg_core.hpp -- the canonical tables of 256 values and the walk over one block's symbols, the lines of the JPEG
decoder that meet untrusted bytes -- compiled for the host into tools/jpeg_core_check.cpp with the address and
undefined-behaviour sanitizers and run, as a child process, over every stream of the case table, short ones included, and
over seeded corruptions of them: it prints what tests/jpeg_restatement.py computes, status words and coefficients, and the
sanitizers stay silent.  The same on the corpus of tests/jpeg_mutants.py: every distinct accepted mutant that jpeg.read takes
with its restart intervals (some 4 000: changed tables, sizes, quantisation selectors, DRI values and restart layouts among
them, before any of them is given to the GPU).  The sanitizer runtimes are linked statically, so the program does not care what else the process
loads and the child inherits the environment as it is.  Where no compiler links them the program is built plain."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "jpeg_core_check.cpp")


def _compilers():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        path = shutil.which(name) if name else None
        if path:
            yield path


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(the built program, whether it carries the sanitizers)"""
    assert os.path.exists(os.path.join(ROOT, "shinestacker_amd", "csrc", "jpeg_core.hpp"))
    d = tmp_path_factory.mktemp("core")
    exe = str(d / "jpeg_core_check")
    tried = []
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # (g++ links the runtimes dynamically unless told otherwise; clang links them statically and does not know the g++ flags)
    for flags in (sanitize + ["-static-libasan", "-static-libubsan"], sanitize + ["-static-libsan"], []):
        for cxx in _compilers():
            if flags and ("clang" in os.path.basename(os.path.realpath(cxx))) != ("-static-libsan" in flags):
                continue
            cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", *flags, SOURCE, "-o", exe]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode == 0:
                return exe, bool(flags)
            tried.append((cmd, res.stderr[-2000:]))
    if not tried:
        pytest.skip("no host C++ compiler on this machine")
    pytest.fail(f"tools/jpeg_core_check.cpp does not compile: {tried[-1]}")


def _record(data, h):
    """one scan in the program's format: the bytes of the scan alone, the offsets counted from its start"""
    off = [o - h["scan_off"] for o in h["offsets"]]
    scan = bytes(data[h["scan_off"]:h["offsets"][-1]])
    lines = [f'{h["width"]} {h["height"]} {h["ncomp"]} {h["hmax"]} {h["vmax"]} {h["dri"]} {len(off) - 1} {len(scan)} {scan.hex() or "-"}',
             " ".join(map(str, off)), " ".join(f"{td} {ta}" for _, td, ta in h["scan"])]
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        counts, values = h["tables"].get(key, ([0] * 16, []))
        lines.append(" ".join(map(str, list(counts) + list(values) + [0] * (256 - len(values)))))
    return "\n".join(lines)


def _want(data, h):
    planes, status = R.walk(data, h)
    return status.tolist() + [int(v) for p in planes for v in p.reshape(-1)]


def _streams():
    """(name, bytes, parsed headers): the table, then seeded corruptions that keep the headers and the offsets"""
    out = []
    for case in JC.CASES + [s[0] for s in JC.SHORT]:
        data = case.data()
        out.append((case.name, data, R.parse(data)))
    rng = np.random.default_rng(2024)
    base = [c for c in JC.CASES if c.name in ("37x53-420-dri5", "37x53-444-dri3", "17x33-420-fine", "zrl-runs", "category-15")]
    assert len(base) == 5
    for case in base:
        data, h = case.data(), R.parse(case.data())
        lo, hi = h["scan_off"], h["offsets"][-1]
        for k in range(12):
            m = bytearray(data)
            for _ in range(1 + k % 4):
                at = int(rng.integers(lo, hi))
                m[at] = int(rng.choice([0x00, 0xFF, 0xD0, 0x7F, int(rng.integers(256))]))
            out.append((f"{case.name}-mutant{k}", bytes(m), h))
    # what jpeg.read refuses and a decoder on its own would meet: a DC symbol above 15, an oversubscribed table
    case = JC.CASES[0]
    for name, key, table in (("dc-symbol-17", (0, 0), (JC.DC[0][0], [17] + JC.DC[0][1][1:])),
                             ("oversubscribed", (1, 0), ([3, 5] + [0] * 14, [0x00, 0x01, 0x11, 0x02, 0x03, 0x21, 0x04, 0x31]))):
        h = R.parse(case.data())
        h["tables"] = dict(h["tables"])
        h["tables"][key] = table
        out.append((name, case.data(), h))
    return out


def test_the_core_equals_the_restatement_on_every_stream(program, tmp_path):
    exe, sanitized = program
    streams = _streams()
    dump = tmp_path / "streams.txt"
    dump.write_text("\n".join(_record(data, h) for _, data, h in streams) + "\n")
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (sanitized, res.stderr[-3000:])
    assert res.stderr == "", res.stderr[-3000:]
    got = res.stdout.splitlines()
    assert len(got) == len(streams)
    flags = 0
    for line, (name, data, h) in zip(got, streams):
        want = _want(data, h)
        assert list(map(int, line.split())) == want, name      # (flagged streams too: the core and the restatement take the same bits)
        for s in want[:len(h["offsets"]) - 1]:
            flags |= s
    assert flags == R.NOCODE | R.OVERRUN | R.RUN


def test_the_core_equals_the_restatement_on_the_mutants(program, tmp_path):
    """every distinct (headers, scan bytes) of the corpus that jpeg.read accepts at split=None, of at most
    jpeg_mutants.MAX_SAMPLES samples: status words and every coefficient, flagged intervals included"""
    import jpeg_mutants as M
    exe, sanitized = program
    print("sanitizers:", sanitized)
    todo = {}
    for o in M.outcomes():
        if o.serial and o.restate:
            todo.setdefault(o.key(), o)
    todo = list(todo.values())
    assert len(todo) >= 3000
    dump = tmp_path / "mutants.txt"
    dump.write_text("\n".join(_record(o.data, M.restated(o).h) for o in todo) + "\n")
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (sanitized, res.stderr[-3000:])
    assert res.stderr == "", res.stderr[-3000:]
    got = res.stdout.splitlines()
    assert len(got) == len(todo)
    flags, flagged = 0, 0
    for line, o in zip(got, todo):
        planes, status = M.restated(o).serial
        want = " ".join(map(str, status.tolist() + np.concatenate([p.reshape(-1) for p in planes]).tolist()))
        assert " ".join(line.split()) == want, o.recipe
        flags |= int(np.bitwise_or.reduce(status))
        flagged += bool(status.any())
    assert flags == R.NOCODE | R.OVERRUN | R.RUN and flagged >= 1500, (flags, flagged)
