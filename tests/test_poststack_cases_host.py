"""CPU: the cases of tests/poststack_cases.py, checked from the NumPy restatements so that the GPU sweep over them
(test_gpu_poststack_edges.py) cannot pass on inputs that say nothing.  Everything asserted here is a condition on the inputs:
the restatement must change a minimum share of a case's samples (a uniformly random frame comes back from the denoise
unchanged at h = 10: every neighbour's weight is zero), the declared identity cases must be identities, every table-placement
case must carry the label of the branch it is there for, the saturated frames must be saturated, and the unsharp table must
hold the samples on which a wrong compare, rounding or clip shows.  No kernel runs here and no figure comes from one."""
import importlib

import numpy as np
import pytest

import nlm_restatement as nlm
import poststack_cases as pc

DENOISE_FLOOR = 0.30        # share of the samples the restatement must change: sweep and placement cases with search >= 3
UNSHARP_FLOOR = 0.05        # the same for the unsharp cases with radius >= 1, amount != 0, threshold <= 10
SATURATED_SHARE = 0.20      # share of a `bright` frame's samples at the type's maximum, and of a `dark` frame's at 0
MIN_SAMPLES = 20            # samples per unsharp condition and dtype, over the whole table


def changed_share(img, out):
    return float((out != img).mean())


# ---------------------------------------------------------------- denoise
def test_denoise_table_covers_every_kernel_variant():
    """every TH 0..5 and s in {0, 1, 5, 10} on every sweep shape, both dtypes; the shapes with one row, one column, one pixel"""
    for dt in pc.DTYPES:
        for shape in pc.SWEEP_SHAPES:
            seen = {(c.template // 2, c.search // 2) for c in pc.DENOISE_CASES if c.dtype == dt and c.shape == shape}
            assert seen >= {(t, s) for t in range(6) for s in (0, 1, 5, 10)}, (pc.dtype_name(dt), shape)
        shapes = {c.shape for c in pc.DENOISE_CASES if c.dtype == dt}
        assert shapes >= set(pc.SHAPES)
        assert any(c.template == 8 and c.search == 20 for c in pc.DENOISE_CASES if c.dtype == dt)
        assert any(c.h != int(c.h) and c.shape == (33, 65) for c in pc.DENOISE_CASES if c.dtype == dt)
    assert max(h * w for h, w in pc.SHAPES) <= 70 * 100


def test_denoise_cases_change_enough_or_are_identities():
    short, wrong = [], []
    for c in pc.DENOISE_CASES:
        img, out = pc.denoise_frame(c), pc.denoise_expected(c)
        assert out.dtype == img.dtype and out.shape == img.shape
        share = changed_share(img, out)
        must_be_identity = c.search == 1 or c.shape == (1, 1) or c.kind in ("constant", "checker")
        assert c.identity == must_be_identity, pc.denoise_name(c)
        if c.identity:
            if share != 0.0:
                wrong.append((pc.denoise_name(c), share))
        elif c.group != "bounds" and share < DENOISE_FLOOR:
            short.append((pc.denoise_name(c), round(share, 4)))
        elif share == 0.0:
            short.append((pc.denoise_name(c), share))
    assert not wrong, ("declared identities the restatement changes", wrong)
    assert not short, ("cases the restatement changes too little (share of the samples)", short)


def test_denoise_placement_cases_carry_their_labels():
    """the label from the restatement's table and from the package's (what the library is handed); each at least LDS_MARGIN from
    the limit; both labels for both dtypes; the largest request is 63 644 bytes; the h = 100 table has no zero entry"""
    dn = importlib.import_module("shinestacker_amd.denoise")
    labels = {}
    for dt, h, tpl, srch, branch in pc.PLACEMENT:
        total, table_len = pc.lds_request(dt, h, tpl, srch)
        name = (pc.dtype_name(dt), h, tpl, srch, total)
        assert pc.table_branch(dt, h, tpl, srch) == branch, name
        assert abs(total - pc.LDS_LIMIT) >= pc.LDS_MARGIN, name
        assert dn.weight_table(dt, pc.cv2_h(dt, h), tpl, srch)[0].size == table_len, name
        labels.setdefault(np.dtype(dt), set()).add(branch)
        for shape in pc.PLACEMENT_SHAPES:
            assert any(c.group == "placement" and (c.dtype, c.h, c.template, c.search, c.shape, c.branch) ==
                       (dt, h, tpl, srch, shape, branch) for c in pc.DENOISE_CASES), name
    assert labels == {np.dtype(np.uint8): {"lds", "global"}, np.dtype(np.uint16): {"lds", "global"}}
    for c in pc.DENOISE_CASES:
        assert c.branch is None or pc.table_branch(c.dtype, c.h, c.template, c.search) == c.branch, pc.denoise_name(c)
    assert pc.lds_request(*pc.LARGEST_LDS)[0] == 63644 and pc.lds_request(np.uint16, 3, 11, 21)[0] == 56404
    # no window gives a larger request that still fits: the frame planes grow with both windows, the table with the strength
    fits = [pc.lds_request(np.uint8, h, 7, 21)[0] for h in range(20, 31)]
    assert max(t for t in fits if t <= pc.LDS_LIMIT) == 63644
    full, _ = nlm.weight_table(np.uint8, 100, nlm.NORM_L2, 1, 21)
    assert full.size == 195076 and full.min() > 0 and pc.lds_request(np.uint8, 100, 1, 21)[1] == full.size


def test_denoise_bounds_cases_reach_the_bounds():
    """bright: at least a fifth of the samples at the maximum, dark: at 0, also at the noise of the unsharp cases;
    constant(max): every weight is table[0], so a pixel's sums are (2s + 1)^2 table[0] max -- for uint8 at search 21 within
    0.01 % of 2^31; checkerboard: the distance between patches of
    opposite colour indexes past the table's end"""
    for dt in pc.DTYPES:
        top = pc.vmax_of(dt)
        kinds = {(c.kind, c.template, c.search) for c in pc.DENOISE_CASES if c.group == "bounds" and c.dtype == dt}
        assert kinds >= {(k, t, 21) for k in ("constant", "bright", "dark") for t in (11, 1)} | {("checker", 7, 21)}
        for shape in pc.BOUNDS_SHAPES:
            share = float((pc.frame("bright", shape, dt, pc.seed_of(shape)) == top).mean())
            assert share >= SATURATED_SHARE, ("bright", pc.dtype_name(dt), shape, share)
            share = float((pc.frame("dark", shape, dt, pc.seed_of(shape)) == 0).mean())
            assert share >= SATURATED_SHARE, ("dark", pc.dtype_name(dt), shape, share)
            for kind, value in (("bright", top), ("dark", 0)):
                share = float((pc.frame(kind, shape, dt, pc.seed_of(shape), pc.UNSHARP_AMP) == value).mean())
                assert share >= SATURATED_SHARE, (kind, "unsharp", pc.dtype_name(dt), shape, share)
            assert (pc.frame("constant", shape, dt) == top).all()
            assert set(np.unique(pc.frame("checker", shape, dt))) == {0, top}
        for c in pc.DENOISE_CASES:
            if c.dtype != dt or c.kind != "checker":
                continue
            t = c.template // 2
            n = (2 * t + 1) ** 2
            norm = nlm.NORM_L2 if dt == np.uint8 else nlm.NORM_L1
            table, shift = nlm.weight_table(dt, pc.cv2_h(dt, c.h), norm, c.template, c.search)
            cross = n * 3 * (top * top if dt == np.uint8 else top)
            assert (cross >> shift) >= nlm.first_zero(table), pc.denoise_name(c)
    table, _ = nlm.weight_table(np.uint8, 10, nlm.NORM_L2, 11, 21)
    largest = 441 * int(table[0]) * 255
    assert 2**31 * 0.9999 < largest < 2**31 and largest + 441 * int(table[0]) // 2 < 2**32


# ---------------------------------------------------------------- unsharp
def test_unsharp_table_covers_every_window_and_pair():
    for dt in pc.DTYPES:
        windows = [pc.usr.window_size(dt, r) for r in pc.RADII]
        assert windows == (pc.U8_WINDOWS if dt == np.uint8 else [1, 3, 5, 9, 15, 21, 25, 33]), windows
        for shape in pc.SHAPES:
            seen = {(c.radius, c.amount, c.threshold) for c in pc.UNSHARP_CASES if c.dtype == dt and c.shape == shape}
            assert seen >= {(r,) + p for r in pc.RADII for p in pc.PAIRS}, (pc.dtype_name(dt), shape)
        extreme = {(c.kind, c.radius, c.amount, c.threshold != 0) for c in pc.UNSHARP_CASES if c.dtype == dt and c.group == "extreme"}
        for radius in (4, 0.5):
            for masked in (False, True):
                assert extreme >= {(k, radius, a, masked) for k in ("checker", "columns") for a in (5.0, -0.5)}
                assert extreme >= {(k, radius, 5.0, masked) for k in ("constant", "bright", "dark")}
        for kind in ("bright", "dark"):
            shapes = {c.shape for c in pc.UNSHARP_CASES if c.dtype == dt and c.kind == kind}
            assert shapes == set(pc.BOUNDS_SHAPES), (kind, shapes)


def test_unsharp_cases_change_enough_or_are_identities():
    short, wrong = [], []
    for c in pc.UNSHARP_CASES:
        img, out = pc.unsharp_frame(c), pc.unsharp_expected(c)
        assert out.dtype == img.dtype and out.shape == img.shape
        share = changed_share(img, out)
        if c.group != "extreme":
            assert c.identity == (c.radius == 0.01 or c.amount == 0 or c.threshold == 64 or c.shape == (1, 1)), pc.unsharp_name(c)
        else:
            # constant frames; 0 / max frames at a positive amount (every sharpened sample clips back to 0 or the maximum); one
            # column of the column pattern is all zeros
            assert c.identity == (c.kind == "constant" or (c.kind in ("checker", "columns") and c.amount > 0) or
                                  (c.kind == "columns" and c.shape[1] == 1)), pc.unsharp_name(c)
        if c.identity:
            if share != 0.0:
                wrong.append((pc.unsharp_name(c), share))
        elif c.radius >= 1 and c.threshold <= 10 and share < UNSHARP_FLOOR:
            short.append((pc.unsharp_name(c), round(share, 4)))
        elif c.group == "extreme" and share == 0.0:      # radius 0.5: exempt from the floor, but no extreme case may say nothing
            short.append((pc.unsharp_name(c), share))
    assert not wrong, ("declared identities the restatement changes", wrong)
    assert not short, ("cases the restatement changes too little (share of the samples)", short)


def unsharp_condition_counts(dtype):
    """Samples of the table's frames of one dtype on which a wrong rule shows, counted with float32 NumPy from the blurred frame
    (the restatement's arithmetic, step by step)."""
    top = pc.vmax_of(dtype)
    n = dict.fromkeys(("on the threshold", "one past the threshold", "tie on an even floor", "tie on an odd floor",
                       "truncation differs from rounding", "addWeighted below 0", "addWeighted above the maximum",
                       "masked below 0", "masked above the maximum"), 0)
    for c in pc.UNSHARP_CASES:
        if c.dtype != dtype:
            continue
        fi = pc.unsharp_frame(c).astype(np.float32)
        fb = pc.unsharp_blurred(c.kind, c.shape, c.dtype, c.radius).astype(np.float32)
        if c.threshold == 0:
            s = (fi * np.float32(1.0 + c.amount)).astype(np.float32) + (fb * np.float32(-c.amount)).astype(np.float32)
            assert s.dtype == np.float32
            floor = np.floor(s)
            tie = (s > 0) & (s < top) & (s - floor == 0.5)
            n["tie on an even floor"] += int((tie & (floor % 2 == 0)).sum())
            n["tie on an odd floor"] += int((tie & (floor % 2 == 1)).sum())
            n["addWeighted below 0"] += int((np.rint(s) < 0).sum())
            n["addWeighted above the maximum"] += int((np.rint(s) > top).sum())
        else:
            thr = np.float32(c.threshold * (256 if dtype == np.uint16 else 1))
            diff = fi - fb
            n["on the threshold"] += int((np.abs(diff) == thr).sum())
            n["one past the threshold"] += int((np.abs(diff) == thr + np.float32(1)).sum())
            mask = np.abs(diff) > thr
            val = fi + (np.float32(c.amount) * diff).astype(np.float32)
            assert val.dtype == np.float32
            inside = mask & (val > 0) & (val < top)
            n["truncation differs from rounding"] += int((inside & (val - np.floor(val) >= 0.5)).sum())
            n["masked below 0"] += int((mask & (val <= -1)).sum())
            n["masked above the maximum"] += int((mask & (val >= top + 1)).sum())
    return n


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_unsharp_table_holds_the_samples_that_tell_the_rules_apart(dtype):
    """|image - blurred| exactly on the threshold (left alone) and one past it (sharpened): `>` against `>=`; exact .5 ties of
    the float32 addWeighted sum on an even and on an odd floor: half to even against half up and truncation; masked values with
    a fraction of .5 or more: truncation against rounding; unclipped values under 0 and over the maximum in both branches"""
    counts = unsharp_condition_counts(dtype)
    shortfall = {k: v for k, v in counts.items() if v < MIN_SAMPLES}
    assert not shortfall, (pc.dtype_name(dtype), "conditions with fewer than %d samples" % MIN_SAMPLES, shortfall, counts)
