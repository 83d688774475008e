"""CPU: csrc/ljpeg_core.hpp -- the bit reader and the one-symbol decode of raw_ljpeg, the lines that meet untrusted bytes --
compiled for the host into tools/ljpeg_core_check.cpp with the address and undefined-behaviour sanitizers and run, as a child
process, over every stream of the case table, short streams included: it prints what tests/ljpeg_restatement.py computes,
status and samples, and the sanitizers stay silent.  The sanitizer runtimes are linked statically, so the program does not
care what else the process loads and the child inherits the environment as it is.  Where no compiler links them the program is
built plain."""
import os
import shutil
import subprocess

import pytest

import ljpeg_cases as LC
import ljpeg_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "ljpeg_core_check.cpp")


def _compilers():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        path = shutil.which(name) if name else None
        if path:
            yield path


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(the built program, whether it carries the sanitizers)"""
    assert os.path.exists(os.path.join(ROOT, "shinestacker_amd", "csrc", "ljpeg_core.hpp"))
    d = tmp_path_factory.mktemp("core")
    exe = str(d / "ljpeg_core_check")
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
    pytest.fail(f"tools/ljpeg_core_check.cpp does not compile: {tried[-1]}")


def test_the_core_equals_the_restatement_on_every_stream(program, tmp_path):
    exe, sanitized = program
    records, want = [], []
    for case in LC.CASES + [s[0] for s in LC.SHORT]:
        info = case.write(str(tmp_path / "case.dng"))
        for stream in info["streams"]:
            p = R.parse(stream)
            data = stream[p["scan_off"]:]
            samples, status = R.decode(data, p["tables"], p["precision"], p["lines"], p["x"], p["ncomp"], p["predictor"])
            lines = [f'{p["precision"]} {p["lines"]} {p["x"]} {p["ncomp"]} {p["predictor"]} {len(data)} {data.hex() or "-"}']
            for counts, values in p["tables"]:
                lines.append(" ".join(map(str, list(counts) + list(values) + [0] * (17 - len(values)))))
            records.append("\n".join(lines))
            want.append((case.name, status, samples.reshape(-1).tolist()))
    # the two known answers, as literal bytes
    for k in LC.KNOWN:
        records.append(f'{k["precision"]} {k["lines"]} {k["x"]} {k["ncomp"]} {k["predictor"]} {len(k["data"])} {k["data"].hex()}\n' +
                       "\n".join(" ".join(map(str, LC.KNOWN_TABLE[0] + LC.KNOWN_TABLE[1] + [0] * 5)) for _ in range(2)))
        want.append(("known", 0, [v for row in k["want"] for v in row]))
    dump = tmp_path / "streams.txt"
    dump.write_text("\n".join(records) + "\n")
    res = subprocess.run([exe, str(dump)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (sanitized, res.stderr[-3000:])
    assert res.stderr == "", res.stderr[-3000:]
    got = res.stdout.splitlines()
    assert len(got) == len(want)
    flagged = 0
    for line, (name, status, samples) in zip(got, want):
        vals = list(map(int, line.split()))
        assert vals[0] == status, (name, vals[0], status)
        assert vals[1:] == samples, name       # (flagged streams too: the core and the restatement take the same bits)
        flagged += status != 0
    assert flagged == len(LC.SHORT)
