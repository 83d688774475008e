"""CPU: jpeg.read, the C boundary's argument checks and the two restatements on the seeded corrupt files of tests/jpeg_mutants.py.

    the reader's contract   every mutant is read into a frame or refused on purpose, at split=None, "needed" and "always", with
                            a message that holds the file's path and names a marker or field; nothing else comes out of
                            jpeg.read (no IndexError, struct.error, ValueError, ...) and no warning is emitted
    bounded work            no parse takes more than 20 times the slowest parse of an unmutated base (1 s at least: the
                            margin is for a busy machine) -- the bound of test_dng_mutants_host.py
    the lenient parser      an accepted frame agrees with jpeg_restatement.parse on every field the kernels take
    the C boundary          what the parser accepts, the argument checks of mi_jpeg_decode and mi_jpeg_split_decode accept
    no case is vacuous      the corpus holds what the GPU file (test_gpu_jpeg_mutants.py) relies on, class by class

The corpus is parsed once (jpeg_mutants.outcomes) and restated once (jpeg_mutants.restated) for the whole session.

Sizes on a CPU-only machine, with Pillow (its six bases are left out without it, and the counts asserted below are the ones
without them): 145 bases, 23 912 mutants; accepted 5 139 at split=None, 9 153 at "needed" and at "always", 9 079 of them of
at most jpeg_mutants.MAX_SAMPLES samples, 7 083 distinct (headers, scan bytes); without Pillow 139 bases, 22 996 mutants,
4 837 and 8 848 accepted, 6 828 distinct.  Parsing takes 19 s there (three reads a
mutant, 0.27 ms each), restating every distinct accepted mutant 45 s (6 ms each).  The class counts: `test_no_case_is_vacuous`.
"""
import collections
import ctypes

import numpy as np
import pytest

import jpeg_mutants as M
from shinestacker_amd.errors import ImageLoadError, InvalidOptionError

# What jpeg.read raises on purpose, from its source: every refusal goes through `_refuse`, an InvalidOptionError that names the
# marker or field as its option and carries the path in its details -- the type the refusals of jpeg_cases.REFUSALS pin and the
# one a stacker's jpeg="auto" catches to fall back to the host decoder.  ImageLoadError is what check_status raises for a
# status word, after a decode; it is admitted here as dng.read's is.  (The RuntimeError for a path that does not exist cannot
# come from a file that does.)
REFUSALS = (ImageLoadError, InvalidOptionError)
SLOWER, AT_LEAST = 20.0, 1.0


@pytest.fixture(scope="module")
def outcomes():
    for b in M.bases():
        o = M.base_outcome(b)
        assert o.accepted and o.serial == b.serial and not o.warnings, (b, o.errors)
    return M.outcomes()


@pytest.fixture(scope="module")
def accepted(outcomes):
    """the accepted outcomes of at most MAX_SAMPLES samples, every one restated (once per distinct input of the kernels)"""
    out = [o for o in outcomes if o.accepted and o.restate]
    with M._no_collection():
        for o in out:
            try:
                M.restated(o)
            except Exception as exc:        # noqa: BLE001
                pytest.fail(f"the restatement raised {exc!r} on {o.recipe}")
    return out


def test_read_returns_a_frame_or_refuses_on_purpose_and_names_the_file_and_the_field(outcomes):
    leaks, nameless, warned, order = [], [], [], []
    for o in outcomes:
        if o.warnings:
            warned.append((o.recipe, o.warnings[:2]))
        for split in M.SPLITS:
            err = o.errors[split]
            if err is None:
                continue
            if not isinstance(err, REFUSALS):
                leaks.append((o.recipe, split, o.where[split], repr(err)[:160]))
            elif o.path not in str(err) or not str(getattr(err, "option", None) or getattr(err, "details", "")).strip():
                nameless.append((o.recipe, split, str(err)[:160]))
        # "needed" takes what None takes, "always" what "needed" takes, and the two differ in nothing but where the frame goes
        if (o.frames[None] is not None and o.frames["needed"] is None) or (o.frames["needed"] is None) != (o.frames["always"] is None):
            order.append(o.recipe)
    assert not leaks, (len(leaks), leaks[:10])
    assert not nameless, (len(nameless), nameless[:10])
    assert not warned, (len(warned), warned[:10])
    assert not order, (len(order), order[:10])


def test_the_work_of_a_parse_is_bounded(outcomes):
    """Measured on a shared CPU machine (145 bases, 23 912 mutants, three reads each): the slowest three reads of an unmutated
    base 2.4 to 2.8 ms, the mean of a mutant 0.8 ms, the slowest 9 to 13 ms.  The bound is SLOWER = 20 times the slowest base
    and AT_LEAST = 1 s whatever that gives: 1 s here.  The test prints the three figures of its own run."""
    slowest = max(M.base_outcome(b).seconds for b in M.bases())
    bound = max(AT_LEAST, SLOWER * slowest)
    worst = max(outcomes, key=lambda o: o.seconds)
    print(f"slowest base parse {slowest:.6f} s, slowest mutant parse {worst.seconds:.6f} s {worst.recipe}, bound {bound:.3f} s")
    assert worst.seconds <= bound, (worst.recipe, worst.seconds, bound)
    for o in outcomes:
        for f in o.frames.values():
            if f is not None:       # nothing in a frame has more entries than the file has bytes
                assert f.n_intervals <= o.nbytes and f.span.nbytes <= o.nbytes and len(f.offsets) == f.n_intervals + 1, o.recipe


def _disagreements(o, split, h):
    """the fields of jpeg.read's frame that differ from the lenient parser's headers `h`"""
    f, d, out = o.frames[split], o.frames[split].desc, []
    comps, mx, my = M.R.geometry(h)

    def want(name, got, value):
        if got != value:
            out.append((name, got, value))
    want("size", f.shape, (h["height"], h["width"]))
    want("desc size", (d.height, d.width), (h["height"], h["width"]))
    want("ncomp", (f.ncomp, d.ncomp), (h["ncomp"], h["ncomp"]))
    want("sampling", (f.sampling, (d.hmax, d.vmax)), ((h["hmax"], h["vmax"]),) * 2)
    want("dri", f.dri, h["dri"])
    per = min(h["dri"], mx * my) if h["dri"] >= 1 else mx * my
    want("desc dri", d.dri, per if f.split else h["dri"])
    want("split", f.split, split == "always" or (split == "needed" and not 1 <= h["dri"] <= M.jpeg.MAX_DRI))
    want("intervals", (f.n_intervals, d.n_intervals), (len(h["offsets"]) - 1,) * 2)
    want("offsets", f.offsets.tolist(), [x - h["scan_off"] for x in h["offsets"]])
    end = h["offsets"][-1]
    want("span", bytes(f.span), o.data[h["scan_off"]:max(end, h["scan_off"] + 1)])
    v = h["orientation"]
    want("orientation", f.orientation, v if 1 <= v <= 8 else 1)
    for c in range(h["ncomp"]):
        _, td, ta = h["scan"][c]
        tq = h["comps"][c][3]
        want(f"selectors {c}", (d.tq[c], d.td[c], d.ta[c]), (tq, td, ta))
        pq, nat = h["quant"].get(tq, (None, None))
        want(f"quant {c}", (0, list(d.quant[tq]) if tq < 4 else None), (pq, nat))
        for cls, t in ((0, td), (1, ta)):
            counts, values = h["tables"].get((cls, t), (None, None))
            if counts is None or t > 1:
                out.append((f"table {cls} {t}", "selected", "absent or not selectable"))
                continue
            want(f"counts {cls} {t}", list(d.counts[2 * cls + t]), list(counts))
            want(f"values {cls} {t}", list(d.values[2 * cls + t])[:len(values)], list(values))
    return out


def test_an_accepted_frame_agrees_with_the_lenient_parser(outcomes):
    """size, sampling, selectors, tables, quantisation, DRI, offsets, span and orientation, at every `split`; the lenient parser
    runs once per accepted mutant"""
    wrong, n = [], collections.Counter()
    for o in outcomes:
        if not o.accepted:
            continue
        try:
            h = M.R.parse(o.data)
        except Exception as exc:        # noqa: BLE001
            wrong.append((o.recipe, "the lenient parser raised", repr(exc)))
            continue
        for split in M.SPLITS:
            if o.frames[split] is not None:
                n[split] += 1
                bad = _disagreements(o, split, h)
                if bad:
                    wrong.append((o.recipe, split, bad[:3]))
    assert not wrong, (len(wrong), wrong[:8])
    assert n[None] >= 4500 and n["needed"] == n["always"] >= 8000, n


def test_what_the_parser_accepts_the_c_boundary_accepts(hiplib, outcomes):
    """the host forms: the argument checks must not answer MI_ERR_INVALID.  Without a device the call then ends at the device
    lookup.  With one it would go on and run the kernels on thousands of corrupt frames from a test that is not marked `gpu`:
    there the test is skipped, as test_dng_mutants_host.py skips its own, and test_gpu_jpeg_mutants.py calls the same host
    forms, checks included, on the mutants it runs."""
    if hiplib.device_count():
        pytest.skip("a GPU is visible here: the host forms would run the kernels (test_gpu_jpeg_mutants.py calls them)")
    lib, seen, calls = hiplib.load(), set(), collections.Counter()
    for o in outcomes:
        if not o.accepted or not o.restate:
            continue
        for split in (None, "always"):
            f = o.frames[split]
            if f is None or (o.key(), split) in seen:
                continue
            seen.add((o.key(), split))
            h, w = f.shape
            out, status = np.zeros((h, w, 3), np.uint8), np.zeros(f.n_intervals, np.uint32)
            span = np.ascontiguousarray(f.span)
            if f.split:
                opt = hiplib.JpegSplitStruct()
                rc = lib.mi_jpeg_split_decode(0, span.ctypes.data, span.nbytes, f.offsets.ctypes.data, ctypes.byref(f.desc), ctypes.byref(opt),
                                              out.ctypes.data, status.ctypes.data)
            else:
                rc = lib.mi_jpeg_decode(0, span.ctypes.data, span.nbytes, f.offsets.ctypes.data, ctypes.byref(f.desc), out.ctypes.data,
                                        status.ctypes.data)
            calls[f.split] += 1
            assert rc != hiplib.MI_ERR_INVALID and rc != hiplib.MI_OK, (o.recipe, split, rc, lib.mi_last_error())
            assert not out.any()
    assert min(calls[False], calls[True]) >= 1000, calls


def _table(accepted):
    """{(mode, with restart intervals): Counter of classes} over the distinct accepted mutants"""
    table, seen = collections.defaultdict(collections.Counter), set()
    for o in accepted:
        if o.key() in seen or not M.changed(o):
            continue
        seen.add(o.key())
        for c in M.classes(o):
            table[M.cell(o)][c] += 1
    return table


# Distinct accepted mutants per class of this corpus WITHOUT the Pillow bases, by a CPU run of the restatements, rounded down
# to a round number (with them every count is a little larger): (mode, read with restart intervals) -> class -> at least
AT_LEAST_PER_CLASS = {
    ('420', False): {'differs': 140, 'nocode': 290, 'overrun': 180, 'run': 80, 'dht-move': 20, 'quant': 130, 'marker': 70},
    ('420', True): {'differs': 160, 'nocode': 290, 'overrun': 220, 'run': 80, 'dht-move': 15, 'quant': 130, 'marker': 70},
    ('422', False): {'differs': 130, 'nocode': 210, 'overrun': 160, 'run': 50, 'dht-move': 15, 'quant': 90, 'marker': 60},
    ('422', True): {'differs': 170, 'nocode': 230, 'overrun': 150, 'run': 70, 'dht-move': 15, 'quant': 110, 'marker': 60},
    ('444', False): {'differs': 70, 'nocode': 140, 'overrun': 80, 'run': 100, 'dht-move': 10, 'quant': 70, 'marker': 30},
    ('444', True): {'differs': 140, 'nocode': 170, 'overrun': 140, 'run': 60, 'dht-move': 30, 'quant': 140, 'marker': 30},
    ('grey', False): {'differs': 110, 'nocode': 100, 'overrun': 130, 'run': 20, 'dht-move': 20, 'quant': 50, 'marker': 40},
    ('grey', True): {'differs': 170, 'nocode': 170, 'overrun': 200, 'run': 70, 'dht-move': 15, 'quant': 80, 'marker': 50},
}


def test_no_case_is_vacuous(outcomes, accepted):
    """Every class of jpeg_mutants.CLASSES, for each of 4:4:4, 4:2:2, 4:2:0 and grey, read with and without restart intervals:
    the classes exactly, the counts at AT_LEAST_PER_CLASS.  Observed with the Pillow bases, distinct accepted mutants, for
    (4:2:0, no restart interval): differs 145, nocode 293, overrun 188, run 80, dht-move 23, quant 130, marker 74; the test
    prints the table of its own run."""
    blind = [o for o in outcomes if o.mutant.blind]
    ok = sum(o.accepted for o in blind)
    assert len(blind) >= 8500 and 4 * (len(blind) - ok) >= len(blind) and 10 * ok >= len(blind), (len(blind), ok)
    table = _table(accepted)
    for k in sorted(table):
        print(k, dict(table[k]))
    assert set(table) == {(m, s) for m in M.MODES for s in (False, True)}, sorted(table)
    for k, row in sorted(table.items()):
        assert set(row) == set(M.CLASSES), (k, sorted(set(M.CLASSES) - set(row)))
        for c, n in AT_LEAST_PER_CLASS[k].items():
            assert row[c] >= n, (k, c, row[c])
    # what never reaches a descriptor: a DC category above 15 and an oversubscribed table are refused by name (the sanitized
    # cores decode both in test_jpeg_core_host.py), as are tables 2 and 3, Pq = 1 and a quantisation entry of 0
    refused = collections.Counter()
    for o in outcomes:
        text = str(o.errors["always"])
        for name, frag in (("category", "a DC category is at most 15"), ("overflow", "the counts overflow the code space"),
                           ("selector", "selects a Huffman table the file does not define"), ("pq", "16-bit quantisation tables"),
                           ("entry-0", "a quantisation entry of 0")):
            refused[name] += frag in text
    assert min(refused[k] for k in ("category", "overflow", "selector", "pq", "entry-0")) >= 50, refused
    # a second SOF0 is ignored where it follows the first (T.81 allows one frame header: the first one read is the frame), a
    # mutated Ss / Se / Ah / Al changes nothing in a baseline scan: both are accepted and give the kernels what the base does
    for kind in ("second-sof", "sos-ss", "sos-se", "sos-ah", "sos-al"):
        mine = [o for o in outcomes if o.mutant.kind == kind]
        assert len(mine) >= 20 and all(o.accepted and not M.changed(o) for o in mine), kind


def test_the_device_selection_holds_every_class(accepted):
    """what test_gpu_jpeg_mutants.py runs: at most 300, no input twice, and every class in every cell again -- the selection
    restates only a few candidates per base, so that it holds them is shown here"""
    sel = M.device_selection()
    assert 200 <= len(sel) <= M.DEVICE_LIMIT and len({o.key() for o in sel}) == len(sel)
    assert all(o.accepted and o.restate and M.changed(o) for o in sel)
    table = _table(sel)
    assert set(table) == {(m, s) for m in M.MODES for s in (False, True)}, sorted(table)
    for k, row in sorted(table.items()):
        assert set(row) == set(M.CLASSES), (k, sorted(set(M.CLASSES) - set(row)))
    # changed headers that jpeg.read still accepted: size, DRI, tables, quantisation
    descs = sum(bytes(o.frame.desc) != bytes(M.base_outcome(o.base).frame.desc) for o in sel)
    assert descs >= 60, descs
    kinds = collections.Counter(o.mutant.kind for o in sel)
    assert kinds["sof-x"] + kinds["sof-y"] >= 1 and kinds["dht-move"] >= 8 and kinds["dqt-entry"] + kinds["second-dqt"] >= 8, kinds
