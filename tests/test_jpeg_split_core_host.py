"""CPU: csrc/jpeg_sync_core.hpp -- the symbol transition and the subsequence walk of the split JPEG decoder, the lines that
meet untrusted bytes -- compiled for the host into tools/jpeg_split_check.cpp with the address and undefined-behaviour
sanitizers and run, as a child process, over every stream of tests/jpeg_split_cases.py, short ones included, and over
seeded corruptions of them, the lanes emulated one after the other as kernels_jpeg_split.hpp runs them: it prints what
tests/jpeg_split_restatement.py computes -- status words, coefficients, and every subsequence's exit from its cold state and
from its true entry -- and the sanitizers stay silent.  The same on the corpus of tests/jpeg_mutants.py: every distinct accepted
mutant, files with and without restart intervals, before any of them is given to the GPU.  The sanitizer runtimes are linked statically, so the program does not
care what else the process loads and the child inherits the environment as it is.  Where no compiler links them the program
is built plain."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_restatement as R
import jpeg_split_cases as SC
import jpeg_split_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "jpeg_split_check.cpp")


def _compilers():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        path = shutil.which(name) if name else None
        if path:
            yield path


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(the built program, whether it carries the sanitizers)"""
    assert os.path.exists(os.path.join(ROOT, "shinestacker_amd", "csrc", "jpeg_sync_core.hpp"))
    d = tmp_path_factory.mktemp("core")
    exe = str(d / "jpeg_split_check")
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
    pytest.fail(f"tools/jpeg_split_check.cpp does not compile: {tried[-1]}")


def _record(data, h):
    """one scan in the program's format (that of tools/jpeg_core_check.cpp); a file without DRI is one interval of all MCUs"""
    off = [o - h["scan_off"] for o in h["offsets"]]
    scan = bytes(data[h["scan_off"]:h["offsets"][-1]])
    _, mx, my = R.geometry(h)
    lines = [f'{h["width"]} {h["height"]} {h["ncomp"]} {h["hmax"]} {h["vmax"]} {h["dri"] or mx * my} {len(off) - 1} {len(scan)} {scan.hex() or "-"}',
             " ".join(map(str, off)), " ".join(f"{td} {ta}" for _, td, ta in h["scan"])]
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        counts, values = h["tables"].get(key, ([0] * 16, []))
        lines.append(" ".join(map(str, list(counts) + list(values) + [0] * (256 - len(values)))))
    return "\n".join(lines)


def _packed(state, n):
    if state is S.END:
        return [0, (1 << 12) | (n << 16)]
    p, q, b, k = state
    return [p, q | (b << 3) | (k << 6) | (n << 16)]


def _want(data, h, sub):
    planes, status = S.walk_split(data, h)
    first = status.tolist() + [int(v) for p in planes for v in p.reshape(-1)]
    lanes = []
    for (iv, lo, hi, last), (cold, true) in zip(S.lanes_of(data, h, sub), S.exits(data, h, sub)):
        # (a subsequence behind the end of its interval's data has no cold state in the restatement: the program's is its own)
        lanes.append((_packed(*cold) if lo <= iv.end else None, _packed(*true)))
    return first, lanes


def _streams():
    """(name, bytes, parsed headers): the tables, then seeded corruptions that keep the headers and the offsets"""
    out = []
    for case in SC.PLAIN + SC.LONG + SC.ALWAYS + [s[0] for s in SC.SHORT]:
        data = case.data()
        out.append((case.name, data, R.parse(data)))
    rng = np.random.default_rng(2025)
    by_name = {c.name: c for c in SC.PLAIN + SC.ALWAYS}
    for name in ("37x53-420", "37x53-444", "17x33-422", "zrl-runs", "category-15", "stuffed-00-first", "37x53-420-dri5"):
        case = by_name[name]
        data, h = case.data(), R.parse(case.data())
        lo, hi = h["scan_off"], h["offsets"][-1]
        for k in range(10):
            m = bytearray(data)
            for _ in range(1 + k % 4):
                at = int(rng.integers(lo, hi))
                m[at] = int(rng.choice([0x00, 0xFF, 0xD0, 0x7F, int(rng.integers(256))]))
            out.append((f"{name}-mutant{k}", bytes(m), h))
    case = by_name["37x53-444"]
    for name, key, table in (("dc-symbol-17", (0, 0), (JC.DC[0][0], [17] + JC.DC[0][1][1:])),
                             ("oversubscribed", (1, 0), ([3, 5] + [0] * 14, [0x00, 0x01, 0x11, 0x02, 0x03, 0x21, 0x04, 0x31]))):
        h = R.parse(case.data())
        h["tables"] = dict(h["tables"])
        h["tables"][key] = table
        out.append((name, case.data(), h))
    return out


@pytest.mark.parametrize("sub", [8, 16, 128])
def test_the_core_equals_the_restatement_on_every_stream(program, tmp_path, sub):
    exe, sanitized = program
    streams = _streams()
    dump = tmp_path / "streams.txt"
    dump.write_text("\n".join(_record(data, h) for _, data, h in streams) + "\n")
    res = subprocess.run([exe, str(dump), str(sub)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (sanitized, res.stderr[-3000:])
    assert res.stderr == "", res.stderr[-3000:]
    got = res.stdout.split("\n")
    assert len(got) == 2 * len(streams) + 1
    flags, compared_cold, differ = 0, 0, 0
    for i, (name, data, h) in enumerate(streams):
        first, lanes = _want(data, h, sub)
        assert list(map(int, got[2 * i].split())) == first, name
        words = list(map(int, got[2 * i + 1].split()))
        assert len(words) == 4 * len(lanes), name
        for j, (cold, true) in enumerate(lanes):
            assert words[4 * j + 2:4 * j + 4] == true, (name, j)
            if cold is not None:
                assert words[4 * j:4 * j + 2] == cold, (name, j)
                compared_cold += 1
                differ += cold != true
        for s in first[:len(h["offsets"]) - 1]:
            flags |= s
    assert flags == S.NOCODE | S.OVERRUN | S.RUN and compared_cold > len(streams)
    assert differ > 0 or sub == 128


LANES_EVERY = 1         # of the mutants, every how-manieth has its subsequences' exits restated and compared as well


@pytest.mark.parametrize("sub", [8, 16, 128])
def test_the_core_equals_the_restatement_on_the_mutants(program, tmp_path, sub):
    """every distinct (headers, scan bytes) of the corpus that jpeg.read accepts, of at most jpeg_mutants.MAX_SAMPLES samples:
    status words, every coefficient and every subsequence's two exits, flagged intervals included"""
    import jpeg_mutants as M
    exe, sanitized = program
    print("sanitizers:", sanitized)
    todo = {}
    for o in M.outcomes():
        if o.accepted and o.restate:
            todo.setdefault(o.key(), o)
    todo = list(todo.values())
    assert len(todo) >= 6000
    dump = tmp_path / "mutants.txt"
    dump.write_text("\n".join(_record(o.data, M.restated(o).h) for o in todo) + "\n")
    res = subprocess.run([exe, str(dump), str(sub)], capture_output=True, text=True, timeout=1800)
    assert res.returncode == 0, (sanitized, res.stderr[-3000:])
    assert res.stderr == "", res.stderr[-3000:]
    got = res.stdout.split("\n")
    assert len(got) == 2 * len(todo) + 1
    flags, flagged, compared = 0, 0, 0
    for i, o in enumerate(todo):
        r = M.restated(o)
        planes, status = r.split
        want = " ".join(map(str, status.tolist() + np.concatenate([p.reshape(-1) for p in planes]).tolist()))
        assert " ".join(got[2 * i].split()) == want, o.recipe
        flags |= int(np.bitwise_or.reduce(status))
        flagged += bool(status.any())
        if i % LANES_EVERY == 0:
            words = list(map(int, got[2 * i + 1].split()))
            lanes = S.lanes_of(o.data, r.h, sub)
            assert len(words) == 4 * len(lanes), o.recipe
            for j, ((iv, lo, hi, last), (cold, true)) in enumerate(zip(lanes, S.exits(o.data, r.h, sub))):
                assert words[4 * j + 2:4 * j + 4] == _packed(*true), (o.recipe, j)
                if lo <= iv.end:
                    assert words[4 * j:4 * j + 2] == _packed(*cold), (o.recipe, j)
                    compared += 1
    assert flags == S.NOCODE | S.OVERRUN | S.RUN and flagged >= 2500 and compared > len(todo) // LANES_EVERY, (flags, flagged, compared)
