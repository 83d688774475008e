"""CPU: csrc/ljpeg_sync_core.hpp -- the symbol transition and the subsequence walk of the split lossless-JPEG decoder, the lines
that meet untrusted bytes -- compiled for the host into tools/ljpeg_split_check.cpp with the address and undefined-behaviour
sanitizers and run, as a child process, over every segment of tests/ljpeg_split_cases.py, short streams included, and over
seeded corruptions of them, the lanes emulated one after the other as kernels_ljpeg_split.hpp runs them: it prints what
tests/ljpeg_split_restatement.py computes -- the status word, the differences, and every subsequence's exit from its cold state
and from its true entry -- and the sanitizers stay silent.  The same on the corrupt files of tests/dng_mutants.py: every segment
of every one- and two-component mutant that dng.read accepts (changed precisions, predictors and DHT counts, `dht-move`,
markers in the middle of a tile, data that ends early, spans declared short), which until now reached the serial core only.
The sanitizer runtimes are linked statically, so the program does
not care what else the process loads and the child inherits the environment as it is.  Where no compiler links them the
program is built plain."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ljpeg_split_cases as SC
import ljpeg_split_restatement as S
from shinestacker_amd import dng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "ljpeg_split_check.cpp")


def _compilers():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        path = shutil.which(name) if name else None
        if path:
            yield path


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(the built program, whether it carries the sanitizers)"""
    assert os.path.exists(os.path.join(ROOT, "shinestacker_amd", "csrc", "ljpeg_sync_core.hpp"))
    d = tmp_path_factory.mktemp("core")
    exe = str(d / "ljpeg_split_check")
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
    pytest.fail(f"tools/ljpeg_split_check.cpp does not compile: {tried[-1]}")


@pytest.fixture(scope="module")
def segments(tmp_path_factory):
    """[(name, Segment, its descriptor)]: every segment of every case, then seeded corruptions of a handful of spans"""
    d = tmp_path_factory.mktemp("ljpeg_split_core")
    out = []
    rng = np.random.default_rng(2027)
    for c in SC.ALL:
        c.write(str(d / (c.name + ".dng")))
        frame = dng.read(str(d / (c.name + ".dng")))
        spans = [(c.name, bytes(frame.span))]
        if c.name in SC.MUTATED:
            spans += [(f"{c.name}-mutant{k}", m) for k, m in enumerate(SC.mutants(bytes(frame.span), frame.layout, rng))]
        for name, span in spans:
            for k, seg in enumerate(S.segments_of(np.frombuffer(span, np.uint8), frame.layout)):
                out.append((f"{name}[{k}]", seg, frame.layout.segments[k]))
    return out


def _record(seg, rec):
    raw = seg.data.raw
    lines = [f"{seg.ncomp} {seg.rows} {seg.cols} {len(raw)} {raw.hex() or '-'}"]
    for c in range(seg.ncomp):
        lines.append(" ".join(map(str, rec["counts"][c].tolist() + rec["values"][c].tolist())))
    return "\n".join(lines)


def _packed(state, n):
    if state is S.END:
        return [0, (1 << 4) | (n << 16)]
    p, q, c = state
    return [p, q | (c << 3) | (n << 16)]


@pytest.mark.parametrize("sub", [8, 16, 128])
def test_the_core_equals_the_restatement_on_every_segment(program, segments, tmp_path, sub):
    exe, sanitized = program
    dump = tmp_path / "segments.txt"
    dump.write_text("\n".join(_record(seg, rec) for _, seg, rec in segments) + "\n")
    res = subprocess.run([exe, str(dump), str(sub)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (sanitized, res.stderr[-3000:])
    assert res.stderr == "", res.stderr[-3000:]
    got = res.stdout.split("\n")
    assert len(got) == 2 * len(segments) + 1
    flags, differ = 0, 0
    for i, (name, seg, _) in enumerate(segments):
        diff, status = S.differences(seg)
        first = np.array(got[2 * i].split(), np.int64)
        assert first[0] == status, name
        assert np.array_equal(first[1:], diff.reshape(-1)), name
        words = list(map(int, got[2 * i + 1].split()))
        lanes = S.exits([seg], sub)
        assert len(words) == 4 * len(lanes), name
        for j, (cold, true) in enumerate(lanes):
            assert words[4 * j + 2:4 * j + 4] == _packed(*true), (name, j)
            # (a subsequence behind the end of its segment's data has no cold state in the restatement: the program's is its own)
            if j * sub <= seg.data.end:
                assert words[4 * j:4 * j + 2] == _packed(*cold), (name, j)
                differ += cold != true
        flags |= status
    assert flags == S.NOCODE | S.OVERRUN
    assert differ > 0


@pytest.mark.parametrize("sub", [8, 128])
def test_the_core_equals_the_restatement_on_the_mutants(program, tmp_path, sub):
    """The corrupt files of tests/dng_mutants.py, deduplicated as test_ljpeg_core_host.py does it: every segment of every one- and
    two-component mutant that dng.read accepts, of every restated base, whose descriptors or span differ from the base's, the
    data as the descriptor states it; a frame once per dng_mutants key, a segment once per record.  The status word, every
    difference and every subsequence's two exits equal the restatement's, and the sanitizers stay silent."""
    import dng_mutants as M
    exe, sanitized = program
    print("sanitizers:", sanitized)
    frames, records, todo = set(), set(), []
    with M._no_collection():
        for o in M.outcomes():
            if not o.accepted or not o.base.restate:
                continue
            lay = o.frame.layout
            if lay.compression != 7 or lay.spp == 3 or not M.changed(o) or o.key() in frames:
                continue
            frames.add(o.key())
            for k, seg in enumerate(S.segments_of(o.frame.span, lay)):
                record = _record(seg, lay.segments[k])
                if record not in records:
                    records.add(record)
                    todo.append((o.recipe, k, seg, record))
    print(f"{len(frames)} accepted frames, {len(todo)} distinct segments")
    assert len(frames) >= 3000, len(frames)
    dump = tmp_path / "mutants.txt"
    dump.write_text("\n".join(t[3] for t in todo) + "\n")
    res = subprocess.run([exe, str(dump), str(sub)], capture_output=True, text=True, timeout=1800)
    assert res.returncode == 0, (sanitized, res.stderr[-3000:])
    assert res.stderr == "", res.stderr[-3000:]
    got = res.stdout.split("\n")
    assert len(got) == 2 * len(todo) + 1
    flagged = {S.NOCODE: 0, S.OVERRUN: 0}
    for i, (recipe, k, seg, _) in enumerate(todo):
        diff, status = S.differences(seg)
        first = np.array(got[2 * i].split(), np.int64)
        assert first[0] == status, (recipe, k)
        assert np.array_equal(first[1:], diff.reshape(-1)), (recipe, k)
        words = list(map(int, got[2 * i + 1].split()))
        lanes = S.exits([seg], sub)
        assert len(words) == 4 * len(lanes), (recipe, k)
        for j, (cold, true) in enumerate(lanes):
            assert words[4 * j + 2:4 * j + 4] == _packed(*true), (recipe, k, j)
            if j * sub <= seg.data.end:
                assert words[4 * j:4 * j + 2] == _packed(*cold), (recipe, k, j)
        for bit in flagged:
            flagged[bit] += bool(status & bit)
    assert min(flagged.values()) >= 300, flagged
