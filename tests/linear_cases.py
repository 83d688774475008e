"""A LinearRaw DNG writer and the case tables shared by test_linear_host.py (CPU: the parser reads what was written, every case
hits the path it names) and test_gpu_linear.py (GPU: the kernels equal the restatements on them).

The writer stands on dng_cases.write_dng: a LinearRaw IFD stores chunky rows, H x W x spp samples, which ARE the H x (W spp)
plane write_dng packs; what differs is the tags -- PhotometricInterpretation 34892, SamplesPerPixel, one BitsPerSample per
sample, widths in pixels, no CFA tag -- and those go in through `extra` and `drop`.

linear_develop's geometry (csrc/kernels_linear.hpp, the constants through shinestacker_amd._lib): the frame is one flat run of
H * W pixels; a group is 4 / itemsize pixels; a workgroup takes _lib.linear_span(dtype) pixels; a group is taken whole ("wide")
when both base pointers are 4-byte aligned and the group ends inside the frame, else sample by sample ("ragged": the frame's
last group; "unaligned": every group behind a base pointer off a 4-byte boundary).

raw_ljpeg3's cases (csrc/kernels_ljpeg.hpp: a batch is 192 samples, 64 whole pixels) stand on ljpeg_cases: its encoder takes
ncomp = 3 and its compressed-DNG writer the same `extra` and `drop`."""
import numpy as np

import dng_cases as D

CFA_TAGS = (33421, 33422, 50710, 50711)
LINEAR = 34892


def write_linear(path, stored, bits, spp=3, tile=None, active_area=None, white=None, black=None, extra=None, drop=(), **kw):
    """Write `stored` (H x W x spp ints below 2^bits; H x W at spp 1) as an uncompressed LinearRaw DNG.  tile: (length, width)
    in pixels; active_area: (top, left, bottom, right) in pixels; white / black: one value or one per sample.  Everything else
    as dng_cases.write_dng (rows_per_strip, order, gap, odd_start, sub_ifd, e, neutral, matrices, table, opcodes2, opcodes3,
    orientation)."""
    a = np.asarray(stored, np.int64)
    h, w = a.shape[:2]
    assert a.shape == ((h, w, spp) if spp != 1 or a.ndim == 3 else (h, w))
    tags = {256: (4, [w]), 262: (3, [LINEAR]), 277: (3, [spp]), 258: (3, [bits] * spp)}
    if tile is not None:
        tags[322] = (4, [tile[1]])
    if active_area is not None:
        tags[50829] = (4, list(active_area))
    if white is not None:
        tags[50717] = (4, [int(v) for v in np.atleast_1d(white)])
    if black is not None:
        tags[50713] = (3, [1, 1])
        tags[50714] = (4, [int(v) for v in np.atleast_1d(black)])
    tags.update(extra or {})
    return D.write_dng(path, a.reshape(h, w * spp), bits, tile=None if tile is None else (tile[0], tile[1] * spp), extra=tags,
                       drop=tuple(CFA_TAGS) + tuple(drop), **kw)


class FileCase:
    """one LinearRaw file: what is stored and what a reader must return, from the stored samples themselves"""

    def __init__(self, name, h, w, bits, spp=3, **kw):
        self.name, self.h, self.w, self.bits, self.spp, self.kw = name, h, w, bits, spp, kw

    def __repr__(self):
        return self.name

    @property
    def dtype(self):
        return np.dtype(np.uint8 if self.bits == 8 else np.uint16)

    def stored(self):
        top = (1 << self.bits) - 1
        rng = np.random.default_rng([self.h, self.w, self.bits, self.spp, 43])
        a = rng.integers(0, top + 1, size=(self.h, self.w, self.spp), dtype=np.int64)
        a.flat[0], a.flat[-1] = top, 0
        return a if self.spp == 3 else a[:, :, 0]

    def whites(self):
        w = [int(v) for v in np.atleast_1d(self.kw.get("white", (1 << self.bits) - 1))]
        return w * self.spp if len(w) == 1 else w

    def blacks(self):
        b = [int(v) for v in np.atleast_1d(self.kw.get("black", 0))]
        return b * self.spp if len(b) == 1 else b

    def shift(self):
        return max(0, 8 * self.dtype.itemsize - max(self.whites()).bit_length())

    def crop(self):
        aa = self.kw.get("active_area")
        return (0, 0, self.h, self.w) if aa is None else (aa[0], aa[1], aa[2] - aa[0], aa[3] - aa[1])

    def expected(self):
        """the samples dng.unpack must return: crop, table (index clamped), shift"""
        top, left, ch, cw = self.crop()
        v = self.stored()[top:top + ch, left:left + cw]
        table = self.kw.get("table")
        if table is not None:
            v = np.asarray(table, np.int64)[np.minimum(v, len(table) - 1)]
        return ((v << self.shift()) & int(np.iinfo(self.dtype).max)).astype(self.dtype)

    def linear_ints(self):
        """(black[spp], gain_q[spp]) a reader must quantise: gain = wb * maxv / ((white - black) << shift), wb = n[1] / n[c]"""
        maxv, s = int(np.iinfo(self.dtype).max), self.shift()
        n = self.kw.get("neutral")
        gq = []
        for c in range(self.spp):
            wb = 1.0 if n is None or self.spp == 1 else float(D.rational(n[1])[0]) / float(D.rational(n[c])[0])
            gq.append(int(np.floor(wb * maxv / float((self.whites()[c] - self.blacks()[c]) << s) * 4096.0 + 0.5)))
        return [b << s for b in self.blacks()], gq

    def write(self, path):
        return write_linear(path, self.stored(), self.bits, spp=self.spp, **self.kw)


FILE_CASES = [
    FileCase("16bit-rgb-5x17", 5, 17, 16),
    FileCase("16bit-rgb-be-5x17", 5, 17, 16, e=">"),
    FileCase("8bit-rgb-5x17", 5, 17, 8),
    FileCase("12bit-rgb-5x17", 5, 17, 12),
    FileCase("14bit-rgb-1x1", 1, 1, 14),
    FileCase("10bit-rgb-7x3-strips-of-2", 7, 3, 10, rows_per_strip=2, order=(3, 1, 0, 2), gap=3, odd_start=True),
    FileCase("12bit-grey-5x17", 5, 17, 12, spp=1),
    FileCase("8bit-grey-3x9", 3, 9, 8, spp=1),
    FileCase("16bit-rgb-sub-ifd", 6, 10, 16, sub_ifd=True, neutral=(0.5, 1.0, 0.625), matrices={2: (D.XYZ_D65_MATRIX, 21)}),
    FileCase("12bit-rgb-levels-per-sample", 6, 10, 12, black=(256, 260, 258), white=(4000, 4095, 3900), neutral=(0.6, 1.0, 0.7)),
    FileCase("12bit-rgb-levels-single", 6, 10, 12, black=(64,), white=(4000,)),
    FileCase("12bit-grey-levels", 6, 10, 12, spp=1, black=(64,), white=(4000,), neutral=(0.6, 1.0, 0.7)),
    FileCase("14bit-rgb-active-area", 12, 20, 14, active_area=(2, 3, 11, 18)),
    FileCase("12bit-rgb-tiles-21x37-active-area", 21, 37, 12, tile=(16, 16), order=(5, 0, 3, 1, 4, 2), gap=7, active_area=(3, 18, 20, 36)),
    FileCase("8bit-rgb-tiles-21x37", 21, 37, 8, tile=(16, 16)),
    FileCase("12bit-rgb-table", 5, 17, 12, table=D._ramp_table(3000)),
]
FILES = {c.name: c for c in FILE_CASES}
assert len(FILES) == len(FILE_CASES)


# ------------------------------------------------------------------------------------------------ linear_develop's shapes
def kernel_shapes(dtype, span):
    """{name: (H, W)}: the frames linear_develop is run on for `dtype`, `span` = the pixels of one workgroup.  The kernel has no
    grid-stride loop -- one workgroup per span, as many as the frame needs -- so "two rows more than a grid step" is aimed at
    two whole spans plus two rows; a grid-stride form would have to re-aim it at its grid's step."""
    shapes = {"1x1": (1, 1), "1xN": (1, 37), "Nx1": (37, 1)}
    shapes.update({f"3x{w}": (3, w) for w in range(1, 10)})
    shapes.update({"span-1": (1, span - 1), "span": (1, span), "span+1": (1, span + 1), "two-rows-past-two-spans": (2 * span // 64 + 2, 64)})
    return shapes


def kernel_paths(h, w, dtype, span, src_misaligned=False, dst_misaligned=False):
    """the paths a frame reaches, from the geometry alone: "wide", "ragged", "unaligned", "second workgroup" """
    px = 4 // np.dtype(dtype).itemsize
    npx = h * w
    seen = set()
    if src_misaligned or dst_misaligned:
        seen.add("unaligned")
    else:
        if npx >= px:
            seen.add("wide")
        if npx % px:
            seen.add("ragged")
    if npx > span:
        seen.add("second workgroup")
    return seen


def samples_for(h, w, spp, dtype, black, white, seed=0):
    """H x W x spp samples (H x W at spp 1) over the dtype's full range, with samples below black, at white and at the dtype's
    maximum among the first pixels"""
    maxv = int(np.iinfo(dtype).max)
    rng = np.random.default_rng([h, w, spp, maxv, seed])
    a = rng.integers(0, maxv + 1, size=(h, w, spp), dtype=np.int64)
    special = [max(0, min(black) - 1), 0, white, maxv, min(black), max(black) + 1]
    flat = a.reshape(-1)
    n = min(len(flat), len(special))
    flat[:n] = special[:n]
    a = a.astype(dtype)
    return a if spp == 3 else a[:, :, 0]


MATRIX = ((1.6, -0.4, -0.2), (-0.3, 1.5, -0.2), (0.1, -0.6, 1.5))


# ------------------------------------------------------------------------------------------------ three-component lossless JPEG
import ljpeg_cases as LJ  # noqa: E402

BATCH3_PX = 64          # ljpeg::BATCH3 / 3 of csrc/kernels_ljpeg.hpp: the pixels of one batch (one per lane)


def write_linear_ljpeg(path, stored, bits, tile=None, active_area=None, extra=None, **kw):
    """Write `stored` (H x W x 3 ints) as a LinearRaw DNG with Compression 7: every strip or tile one SOF3 stream of Nf = 3
    with X the segment's pixel width (ljpeg_cases.encode).  tile, active_area: in pixels; everything else as
    ljpeg_cases.write_dng (predictor, precision, tables, rows_per_strip, order, gap, odd_start, mangle, white, table, ...)."""
    a = np.asarray(stored, np.int64)
    h, w = a.shape[:2]
    assert a.shape == (h, w, 3)
    tags = {256: (4, [w]), 262: (3, [LINEAR]), 277: (3, [3]), 258: (3, [bits] * 3)}
    if tile is not None:
        tags[322] = (4, [tile[1]])
    if active_area is not None:
        tags[50829] = (4, list(active_area))
    tags.update(extra or {})
    return LJ.write_dng(path, a.reshape(h, 3 * w), bits, ncomp=3, tile=None if tile is None else (tile[0], 3 * tile[1]), extra=tags,
                        drop=CFA_TAGS, **kw)


class Ljpeg3Case(LJ.Case):
    """h x w PIXELS of three samples; the samples come from ljpeg_cases.Case.stored on the h x 3w plane"""

    def __init__(self, name, h, w, bits, **kw):
        self.tile_px, self.area_px = kw.pop("tile", None), kw.pop("active_area", None)
        super().__init__(name, h, 3 * w, bits, ncomp=3, **kw)
        self.wpx = w

    def crop_px(self):
        return (0, 0, self.h, self.wpx) if self.area_px is None else (self.area_px[0], self.area_px[1], self.area_px[2] - self.area_px[0],
                                                                    self.area_px[3] - self.area_px[1])

    def expected_px(self):
        """H x W x 3 of what dng.unpack must return: crop, table (index clamped), shift"""
        top, left, ch, cw = self.crop_px()
        v = self.stored().reshape(self.h, self.wpx, 3)[top:top + ch, left:left + cw]
        table = self.kw.get("table")
        if table is not None:
            v = np.asarray(table, np.int64)[np.minimum(v, len(table) - 1)]
        return ((v << self.shift()) & int(np.iinfo(self.dtype).max)).astype(self.dtype)

    def write(self, path):
        return write_linear_ljpeg(path, self.stored().reshape(self.h, self.wpx, 3), self.bits, tile=self.tile_px, active_area=self.area_px,
                                  predictor=self.predictor, precision=self.precision, **self.kw)


LJPEG3_CASES = [
    Ljpeg3Case("12bit-one-pixel", 1, 1, 12),
    Ljpeg3Case("12bit-2x2", 2, 2, 12),
    Ljpeg3Case("12bit-3x63-one-batch-minus-one", 3, BATCH3_PX - 1, 12),
    Ljpeg3Case("12bit-3x64-one-batch", 3, BATCH3_PX, 12, fill="smooth"),
    Ljpeg3Case("12bit-3x65-one-batch-plus-one", 3, BATCH3_PX + 1, 12),
    Ljpeg3Case("14bit-3x129-two-batches-plus-one", 3, 2 * BATCH3_PX + 1, 14, fill="smooth"),
    Ljpeg3Case("16bit-file-12bit-precision", 5, 18, 16, precision=12, white=4095),
    Ljpeg3Case("14bit-strips-of-3-short-last", 7, 18, 14, predictor=2, rows_per_strip=3, order=(2, 0, 1), gap=5),
    Ljpeg3Case("12bit-tiles-21x37-shuffled-active-area", 21, 37, 12, tile=(16, 16), order=(5, 0, 3, 1, 4, 2), gap=7, odd_start=True,
               fill="smooth", active_area=(3, 18, 20, 36)),
    Ljpeg3Case("8bit-tiles-21x37-p5", 21, 37, 8, predictor=5, tile=(16, 16)),
    Ljpeg3Case("16bit-flip-32768-all-stuffed", 4, 200, 16, fill="flip", tables=LJ.LONG_TABLE),
    Ljpeg3Case("16bit-long-codes-p5", 6, 40, 16, predictor=5, tables=LJ.LONG_TABLE_REVERSED, fill="smooth"),
    Ljpeg3Case("12bit-table-short", 5, 18, 12, table=D._ramp_table(3000)),
    Ljpeg3Case("16bit-40x70-random-long-stream", 40, 70, 16),
]
for _p in range(1, 8):
    LJPEG3_CASES.append(Ljpeg3Case(f"12bit-7x{66 + _p}-p{_p}", 7, 66 + _p, 12, predictor=_p, fill="smooth" if _p % 2 else "random"))
LJPEG3 = {c.name: c for c in LJPEG3_CASES}
assert len(LJPEG3) == len(LJPEG3_CASES)

# a stream cut short: (case, the segment that is flagged, its flag)
LJPEG3_SHORT = (Ljpeg3Case("short-cut-mid-data", 9, 18, 12, rows_per_strip=3, mangle=LJ._cut), 1, 2)
