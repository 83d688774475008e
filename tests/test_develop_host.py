"""CPU: no development case of tests/develop_cases.py is vacuous -- on the restatement alone the matrices clamp at both ends,
every number of valid neighbours occurs, the k = 3 case rounds up, the random tone table is not monotonic and the row at the
bound fits int32 -- and Develop, the tone helpers and defects_from_dark validate and quantise as documented."""
import numpy as np
import pytest

import develop_cases as vc
import develop_restatement as DR
from shinestacker_amd import Develop, InvalidOptionError
from shinestacker_amd import demosaic as D
from shinestacker_amd.errors import BitDepthError


def is_permutation(mq):
    m = np.array(mq).reshape(3, 3)
    return set(mq) == {0, 4096} and (m.sum(axis=0) == 4096).all() and (m.sum(axis=1) == 4096).all()


@pytest.mark.parametrize("dtype", vc.DTYPES)
@pytest.mark.parametrize("name", [n for n in vc.MATRICES if n != "identity"])
def test_every_matrix_case_clamps_at_both_ends(name, dtype):
    """On the demosaiced random mosaic of the ragged shape, sums below 0 and sums above white both occur.  A permutation's
    sums are its inputs and never leave [0, white]: there the output must sit ON both bounds and differ from its input."""
    mx = int(np.iinfo(dtype).max)
    bgr = vc.dc.reference(vc.RAGGED, dtype, "GRBG")
    mq = DR.quantise_matrix(vc.MATRICES[name])
    out, pre = DR.colour_matrix(bgr, mq, mx, return_sums=True)
    assert out.min() == 0 and out.max() == mx
    if is_permutation(mq):
        assert np.array_equal(pre, out) and not np.array_equal(out, bgr)
        assert np.array_equal(out[..., 2], bgr[..., 0])        # R out = B in (row 0 = [0, 0, 1])
    else:
        assert (pre < 0).sum() > 0 and (pre > mx).sum() > 0, (int((pre < 0).sum()), int((pre > mx).sum()))
    if name == "zero row":
        assert not out[..., 2].any() and out[..., 1].any()      # row 0 is R's


def test_identity_matrix_is_the_identity():
    for dtype in vc.DTYPES:
        bgr = vc.dc.reference(vc.RAGGED, dtype, "RGGB")
        assert np.array_equal(DR.colour_matrix(bgr, DR.quantise_matrix(vc.MATRICES["identity"]), np.iinfo(dtype).max), bgr)


def test_the_row_at_the_bound_fits_int32():
    mq = np.array(DR.quantise_matrix(vc.MATRICES["row at the bound"]), dtype=np.int64).reshape(3, 3)
    assert np.abs(mq).sum(axis=1).max() == DR.ROW_BOUND == D.MATRIX_ROW_BOUND and np.abs(mq[0]).sum() == DR.ROW_BOUND
    # the extreme sums: every positive entry meets the maximum and every negative one 0, and the reverse; int32 arithmetic
    # (wrapping products and sums, as the kernel's) equals int64
    for dtype in vc.DTYPES:
        mx = int(np.iinfo(dtype).max)
        for rgb in ([mx, mx, mx], [mx, 0, 0], [0, mx, mx], [mx, 0, mx], [0, mx, 0]):
            v = np.array(rgb, dtype=np.int64)
            want = mq @ v + 2048
            with np.errstate(over="ignore"):
                got = (mq.astype(np.int32) * v.astype(np.int32)).sum(axis=1, dtype=np.int32) + np.int32(2048)
            assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), want), rgb
    assert abs(int(mq[0, 0]) * 65535 + 2048) < 2 ** 31 and DR.ROW_BOUND * 65535 + 2048 < 2 ** 31


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_every_k_occurs_and_the_k3_case_rounds_up(dtype):
    seen = set()
    for i, (name, mosaic, sites) in enumerate(vc.defect_cases(dtype)):
        out, ks, lin = vc.defects_reference(dtype, i)
        seen |= set(int(k) for k in ks)
        flat_in, flat_out = mosaic.reshape(-1), out.reshape(-1)
        keep = np.ones(mosaic.size, dtype=bool)
        keep[lin] = False
        assert np.array_equal(flat_in[keep], flat_out[keep]), name          # unlisted sites are only read
        assert np.array_equal(flat_in[lin[ks == 0]], flat_out[lin[ks == 0]]), name
        if "k = 0" in name:
            assert (ks == 0).any(), name
        if "2 x 2" in name or "3 x 3" in name:
            assert (ks == 0).all() and np.array_equal(out, mosaic)
        if "k = 1" in name:
            assert 1 in ks
        if "k = 2" in name:
            assert (ks == 2).all()
        if name == "three valid neighbours, rounding up":
            w = mosaic.shape[1]
            j = int(np.flatnonzero(lin == 10 * w + 20)[0])
            s = int(mosaic[8, 20]) + int(mosaic[12, 20]) + int(mosaic[10, 18])
            assert ks[j] == 3 and out[10, 20] == (s + 1) // 3 == s // 3 + 1
        if name == "neighbours at the maximum":
            assert (ks == 4).any() and (out == np.iinfo(dtype).max).all()
        if name == "an empty list":
            assert len(lin) == 0 and np.array_equal(out, mosaic)
        if name == "a dense 10 % mask":
            assert 0.08 < len(lin) / mosaic.size < 0.12 and len(set(int(k) for k in ks)) >= 4
        if name == "every edge, second row and column":
            assert (ks < 4).all() and (ks >= 1).all()
        if name == "both sides of a tile boundary":
            ys, xs = np.divmod(lin, mosaic.shape[1])
            assert (ys < vc.TH).any() and (ys >= vc.TH).any() and (xs < vc.TW).any() and (xs >= vc.TW).any()
        if len(lin) and "k = 0" not in name:
            assert not np.array_equal(out, mosaic), name
    assert seen == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_tone_tables(dtype):
    dt = np.dtype(dtype)
    mx = int(np.iinfo(dt).max)
    for name in vc.TONES:
        t = vc.tone_table(name, dt)
        assert t.dtype == dt and t.shape == (mx + 1,)
    assert (np.diff(vc.tone_table("random", dt).astype(np.int64)) < 0).any() and (np.diff(vc.tone_table("random", dt).astype(np.int64)) > 0).any()
    assert np.array_equal(vc.tone_table("identity", dt), np.arange(mx + 1))
    assert np.array_equal(vc.tone_table("reversed", dt), mx - np.arange(mx + 1))
    for name in ("srgb", "gamma 2.2", "white below the maximum"):
        t = vc.tone_table(name, dt).astype(np.int64)
        assert t[0] == 0 and t[-1] == mx and (np.diff(t) >= 0).all() and t[mx // 2] > mx // 2     # the curves brighten
    w = vc.white_below(dt)
    t = vc.tone_table("white below the maximum", dt)
    assert (t[w:] == mx).all() and t[w - 1] < mx
    # the helpers, against their formulas at a few points
    i = np.array([0, 1, mx // 100, mx // 3, mx - 1, mx])
    x = i / mx
    assert np.array_equal(D.gamma_tone(dt, 2.2)[i], np.floor(mx * x ** (1 / 2.2) + 0.5).astype(dt))
    assert np.array_equal(D.gamma_tone(dt, 1.0), np.arange(mx + 1))
    srgb = np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1 / 2.4) - 0.055)
    assert np.array_equal(D.srgb_tone(dt)[i], np.floor(mx * srgb + 0.5).astype(dt))
    for bad in (dict(white=0), dict(white=mx + 1), dict(white=1.5)):
        with pytest.raises(InvalidOptionError):
            D.srgb_tone(dt, **bad)
    for bad in (0, -1.0, float("nan"), "2.2", True):
        with pytest.raises(InvalidOptionError):
            D.gamma_tone(dt, bad)
    with pytest.raises(BitDepthError):
        D.srgb_tone(np.float32)


def test_matrix_quantisation():
    d = Develop(matrix=vc.MATRICES["camera"])
    assert d.matrix_q == DR.quantise_matrix(vc.MATRICES["camera"]) == (7373, -2458, -819, -1229, 6554, -1229, 205, -2253, 6144)
    assert Develop(matrix=np.eye(3)).matrix_q == (4096, 0, 0, 0, 4096, 0, 0, 0, 4096)
    assert Develop(matrix=vc.MATRICES["row at the bound"]).matrix_q[:3] == (16384, -8192, -8191)
    # half a unit rounds up, towards plus infinity
    assert Develop(matrix=[[0.5 / 4096, -0.5 / 4096, 1.5 / 4096], [0, 0, 0], [0, 0, 0]]).matrix_q[:3] == (1, 0, 2)
    assert Develop().matrix_q is None and Develop().tone is None and len(Develop().sites((4, 4))) == 0
    s = Develop(matrix=np.eye(3) * 2)
    assert s.matrix_q[0] == 8192


def test_develop_validation():
    for bad in (np.eye(2), np.zeros((3, 4)), [1.0, 2.0, 3.0], "identity", [[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]]):
        with pytest.raises(InvalidOptionError):
            Develop(matrix=bad)
    over = [[4.0, -2.0, -2.0], [0, 1, 0], [0, 0, 1]]           # 16384 + 8192 + 8192 = 32768
    with pytest.raises(InvalidOptionError):
        Develop(matrix=over)
    Develop(matrix=vc.MATRICES["row at the bound"])            # 32767 passes
    for bad in (np.zeros(255, np.uint8), np.zeros(256, np.uint16), np.zeros(65535, np.uint16), np.zeros((16, 16), np.uint8), "linear", -2.2):
        with pytest.raises(InvalidOptionError):
            Develop(tone=bad)
    with pytest.raises(BitDepthError):
        Develop(tone=np.zeros(256, np.float32))
    with pytest.raises(BitDepthError):                          # a uint8 table for uint16 frames
        Develop(tone=np.arange(256).astype(np.uint8)).tone_table(np.uint16)
    assert Develop(tone="srgb").tone_table(np.uint16).shape == (65536,) and Develop(tone="sRGB").tone_table(np.uint8).dtype == np.uint8
    assert np.array_equal(Develop(tone=2.2).tone_table(np.uint8), D.gamma_tone(np.uint8, 2.2))
    for bad in (np.zeros((3, 3), np.int64), np.zeros((2, 2), np.float64), [1, 2, 3]):
        with pytest.raises(InvalidOptionError):
            Develop(defects=bad)
    # sites: sorted, unique, range-checked against the frame at first use
    d = Develop(defects=[(3, 1), (0, 2), (3, 1), (0, 0)])
    assert d.sites((4, 5)).dtype == np.int32 and d.sites((4, 5)).tolist() == [0, 2, 16]
    assert d.sites((4, 2 + 1)).tolist() == [0, 2, 10]
    for shape in ((3, 5), (4, 2)):
        with pytest.raises(InvalidOptionError):
            d.sites(shape)
    with pytest.raises(InvalidOptionError):
        Develop(defects=[(-1, 0)]).sites((4, 4))
    mask = np.zeros((4, 5), bool)
    mask[1, 2] = mask[3, 4] = True
    assert Develop(defects=mask).sites((4, 5)).tolist() == [7, 19]
    with pytest.raises(InvalidOptionError):
        Develop(defects=mask).sites((5, 4))
    assert np.array_equal(Develop(defects=mask).sites((4, 5)), vc.linear_sites(mask, (4, 5)))


def test_develop_without_mosaic_is_refused():
    """before any device is looked for"""
    from shinestacker_amd import PyramidStack, pipeline
    frames = [np.zeros((64, 64, 3), np.uint8)] * 2
    with pytest.raises(InvalidOptionError):
        PyramidStack().focus_stack_arrays(frames, develop=Develop(tone="srgb"))
    with pytest.raises(InvalidOptionError):
        pipeline.bunches_then_stack(lambda i: frames[i], 2, 64, 64, np.uint8, frames=2, overlap=1, develop=Develop(tone="srgb"))
    with pytest.raises(InvalidOptionError):
        PyramidStack().focus_stack_arrays([f[..., 0] for f in frames], mosaic=D.Cfa(), develop="srgb")
    with pytest.raises(InvalidOptionError):
        D.debayer(np.zeros((4, 4), np.uint8), D.Cfa(), develop="srgb")


def test_defects_from_dark():
    dark = np.zeros((6, 7), np.uint16)
    dark[4, 1], dark[0, 6], dark[2, 3], dark[5, 5] = 900, 70, 64, 65
    sites = D.defects_from_dark(dark, 64)
    assert sites.shape == (3, 2) and sites.tolist() == [[0, 6], [4, 1], [5, 5]]       # above, not at, the threshold; ascending
    assert D.defects_from_dark(dark, 1000).shape == (0, 2)
    assert Develop(defects=sites).sites(dark.shape).tolist() == [6, 29, 40]
    assert Develop(defects=D.defects_from_dark(dark, 1000)).sites(dark.shape).tolist() == []
    with pytest.raises(InvalidOptionError):
        D.defects_from_dark(dark[..., None], 64)
    with pytest.raises(InvalidOptionError):
        D.defects_from_dark(dark, "64")
    with pytest.raises(BitDepthError):
        D.defects_from_dark(dark.astype(np.float32), 64)


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_the_steps_move_the_result(dtype):
    """every full case differs from the plain demosaic and from the same development without its defects"""
    for name, m, cfa, mat, tone, defects in vc.full_cases(dtype):
        t = None if tone is None else vc.tone_table(tone, dtype)
        mm = None if mat is None else vc.MATRICES[mat]
        full = vc.restate(m, cfa, mm, t, defects)
        assert full.dtype == m.dtype and full.shape == m.shape + (3,)
        assert not np.array_equal(full, vc.dc.restate(m, cfa)), name
        assert not np.array_equal(full, vc.restate(m, cfa, mm, t, None)), name
