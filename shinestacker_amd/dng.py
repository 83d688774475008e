"""DNG raw files in: the TIFF structure parsed on the host, the samples -- packed (csrc/kernels_unpack.hpp) or lossless JPEG
(Compression 7, csrc/kernels_ljpeg.hpp) -- unpacked or decoded on the MI355X.

The reference reads developed frames and never opens a raw file, so this has no reference counterpart.  DNG is the documented
raw container and it is a TIFF: `read` walks the IFDs with `struct` and NumPy alone and never touches the sample data -- it
maps the file and hands out `span`, one contiguous uint8 view from the lowest segment offset to the end of the highest, which
is uploaded as it lies.  A 12-bit mosaic is 1.5 bytes per site in the file and 2 once unpacked: the file's bytes are 0.75 of
the mosaic's over the host link, and the host never shuffles a bit.

What a `DngFrame` carries: `layout` (a RawLayout: how samples lie in the span), `cfa` (a demosaic.Cfa from CFAPattern,
BlackLevel, WhiteLevel and AsShotNeutral), `develop` (a demosaic.Develop from the colour matrix, or None), `lens` (a lens.Lens
from the WarpRectilinear opcode, or None), `orientation` (reported; applied by `finish`), `finish` (a Finish: the file's
FixVignetteRadial, default crop and orientation, applied only when asked for) and `ignored`: the names of every tag and
opcode in the file that carries a correction a default read does NOT apply -- nothing is dropped silently.

Lossless JPEG (ITU-T T.81, SOF3, Huffman coded: what most cameras and converters write): every strip or tile is one JPEG
stream; `read` parses each stream's markers out of the mapping -- headers only, a few hundred bytes a tile -- into one
descriptor per segment (`RawLayout.segments`), and the kernel decodes the entropy-coded data.  The compressed bytes are the
smallest form of the frame that can cross the host link.  Accepted: one or two components whose samples interleave along the
segment's rows (X * Nf == the segment's columns), Y equal to the segment's rows, 2 <= P <= BitsPerSample, predictors 1 to 7,
no point transform, no restart interval, one scan.  `unpack` raises ImageLoadError when a stream ends early or holds bits that
match no code; a stack asks its handle (`Stack.ljpeg_status`).

Refused, each with the tag's name and value, before any device call: deflate and lossy JPEG samples, a lossless-JPEG
segment outside the above (each as InvalidOptionError("Compression", 7, "lossless JPEG: segment k: ...")), more than one sample
per pixel in a CFA IFD, a CFA repeat other than 2 x 2, a CFALayout other than 1, bit depths other than 8, 10,
12, 14 and 16, truncated segments, and a TIFF with neither a CFA nor a LinearRaw IFD.

LinearRaw (PhotometricInterpretation 34892: an already demosaiced frame -- raw denoisers, pixel-shift composites, Foveon and
monochrome bodies, a converter's "linear DNG" option) is read when no CFA IFD is there: SamplesPerPixel 1 or 3, chunky
(PlanarConfiguration 1), one bit depth for every sample, BlackLevelRepeatDim (1, 1), BlackLevel and WhiteLevel single or per
sample; the CFA tags are not read, everything else is read as for a mosaic.  `DngFrame.cfa` is then None and
`DngFrame.linear` a demosaic.Linear, quantised as the Cfa is; `DngFrame.shape` stays in pixels and the RawLayout counts
SAMPLES (`RawLayout.spp`): chunky rows of W pixels are rows of W spp samples, so raw_unpack decodes them unchanged, and a
three-sample lossless-JPEG tile is one stream of Nf = 3 that raw_ljpeg3 decodes (descriptors: _lib.LJPEG_SEG3_DTYPE).
`unpack` returns H x W x 3 RGB samples (H x W at one sample), `develop` runs demosaic.develop_linear on them (no demosaic;
colour matrix, tone curve, lens, default crop and orientation as for a mosaic).  What is per CFA site does not apply
(`check_linear_options`): a Calibration, Develop.defects, a SiteCorrections object and a Finish with a vignette raise
InvalidOptionError; the file's own GainMap, bad-pixel opcodes, BlackLevelDeltaH/V and FixVignetteRadial are recorded in
`corrections.skipped` / `finish.skipped` with the reason "LinearRaw frame" and stay in `ignored`.  Refused by name: planar
storage, unequal bit depths, SamplesPerPixel 2 or 4, streams whose Nf is not the frame's.  Stack.push_packed takes a linear
frame through the mosaic stage's one ingest path (mi_stack_push_linear): a slot of H x W x spp samples, linear_develop behind it.

The tag numbers and the opcode layouts (WarpRectilinear, GainMap, FixBadPixelsConstant, FixBadPixelsList) are written from
memory of the DNG specification: this reader is UNPINNED against a real DNG -- it has met only the files its own tests write
(tests/dng_cases.py, written from the format description).  The one formula that places a pixel in an opcode's relative
coordinates is `relative`.

Site corrections (`SiteCorrections`, `DngFrame.corrections`; csrc/kernels_sitecorr.hpp, tests/sitecorr_restatement.py is the
definition): the per-site corrections the file carries for its own samples -- BlackLevelDeltaH/V and, from OpcodeList2, GainMap,
FixBadPixelsList and FixBadPixelsConstant -- applied to the unpacked mosaic on the device, integer and exact, in this order:

    raw_unpack / raw_ljpeg -> file bad sites (list, constant) -> file black deltas + gain maps -> Calibration -> step 0 -> ...

They are OFF unless asked for (`corrections="auto"` on Raw, unpack, develop, frames_device, Stack.push_packed): `ignored` lists
them whether or not they can be applied, `DngFrame.remaining(corrections)` is what is still not applied with them.  A
correction that cannot be used is recorded in `corrections.skipped` with its reason and stays in `ignored`.  Opcode
coordinates in OpcodeList2 are taken as those of the active area, the cropped mosaic.

Finish (`Finish`, `RadialGain`, `DngFrame.finish`; csrc/kernels_finish.hpp, tests/finish_restatement.py is the definition):
FixVignetteRadial of OpcodeList3 as a radial gain on the linear mosaic, DefaultCropOrigin / DefaultCropSize and Orientation
as one last pass over the developed frame.  OFF unless asked for (`finish="auto"` on Raw, unpack, develop, frames_device):

    ... -> file black deltas + gain maps -> radial gain -> Calibration -> step 0 -> demosaic / develop -> lens -> crop + orientation

What cannot be used is recorded in `finish.skipped` with its reason and stays in `ignored`; `DngFrame.remaining(corrections,
finish)` is what is left with both options.  An Orientation outside 1 to 8 is refused.

The sample arithmetic is integer and exact (tests/unpack_restatement.py is its definition):

    v = the sample's bits;  v = table[min(v, len - 1)] with a LinearizationTable;  out = v << shift
    shift = max(0, bits of the dtype - bit_length(WhiteLevel)): a 12-bit sensor fills the top of uint16, so that the Cfa's
    gains (white balance times maxv / (white - black)) stay below 16; black and white move with it

There is no CPU path: without a GPU or the library `unpack` and its kin raise DeviceError.  `read` is host Python.
"""
import math
import os
import struct

import numpy as np

from . import _lib
from .demosaic import PATTERNS, Cfa, Develop, Linear, debayer, debayer_device, develop_linear, develop_linear_device, srgb_tone
from .errors import ImageLoadError, InvalidOptionError

EXTENSIONS = frozenset(["dng"])
BITS = (8, 10, 12, 14, 16)
MAX_TABLE = 65536                               # unpack::MAX_TABLE of csrc/kernels_unpack.hpp
MAX_SUB_IFDS = 64                               # SubIFDs followed in search of the raw IFD (a DNG holds a handful: previews)
XYZ_FROM_SRGB = np.array([[0.4124564, 0.3575761, 0.1804375],
                          [0.2126729, 0.7151522, 0.0721750],
                          [0.0193339, 0.1191920, 0.9503041]], np.float64)
D65 = 21                                        # CalibrationIlluminant: D65

TAG_NAMES = {254: "NewSubFileType", 256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression",
             262: "PhotometricInterpretation", 273: "StripOffsets", 274: "Orientation", 277: "SamplesPerPixel",
             278: "RowsPerStrip", 279: "StripByteCounts", 284: "PlanarConfiguration", 322: "TileWidth", 323: "TileLength",
             324: "TileOffsets", 325: "TileByteCounts", 330: "SubIFDs", 33421: "CFARepeatPatternDim", 33422: "CFAPattern",
             50706: "DNGVersion", 50710: "CFAPlaneColor", 50711: "CFALayout", 50712: "LinearizationTable",
             50713: "BlackLevelRepeatDim", 50714: "BlackLevel", 50715: "BlackLevelDeltaH", 50716: "BlackLevelDeltaV",
             50717: "WhiteLevel", 50718: "DefaultScale", 50719: "DefaultCropOrigin", 50720: "DefaultCropSize",
             50721: "ColorMatrix1", 50722: "ColorMatrix2", 50727: "AnalogBalance", 50728: "AsShotNeutral",
             50778: "CalibrationIlluminant1", 50779: "CalibrationIlluminant2", 50829: "ActiveArea", 51008: "OpcodeList1",
             51009: "OpcodeList2", 51022: "OpcodeList3"}
# tags that carry a correction this reader does not apply: reported in DngFrame.ignored when present
IGNORED_TAGS = (50715, 50716, 50718, 50719, 50720, 50727)
OPCODE_NAMES = {1: "WarpRectilinear", 2: "WarpFisheye", 3: "FixVignetteRadial", 4: "FixBadPixelsConstant", 5: "FixBadPixelsList",
                6: "TrimBounds", 7: "MapTable", 8: "MapPolynomial", 9: "GainMap", 10: "DeltaPerRow", 11: "DeltaPerColumn",
                12: "ScalePerRow", 13: "ScalePerColumn"}
COMPRESSION_NAMES = {7: "lossless JPEG", 8: "deflate", 34892: "lossy JPEG"}
CFA_PHOTOMETRIC = 32803
LINEAR_PHOTOMETRIC = 34892                      # LinearRaw: an already demosaiced frame
LINEAR_REASON = "LinearRaw frame"               # why a per-site correction of a LinearRaw file is skipped
_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2), 9: ("i", 4),
          10: ("ii", 8), 11: ("f", 4), 12: ("d", 8), 13: ("I", 4)}
_INTEGRAL = frozenset((1, 3, 4, 6, 8, 9, 13))   # the TIFF types whose values are ints


class RawLayout:
    """How the samples of a raw IFD lie in `DngFrame.span` (mi_raw_layout_t plus the offsets and the table).

    bits                        8, 10, 12, 14 or 16 bits per sample
    big_endian                  the file's byte order; it matters for 16-bit samples only (10, 12 and 14-bit samples are packed
                                most significant bit first whatever the file's order: TIFF FillOrder 1)
    image_height, image_width   the stored image
    tiled                       False: strips of seg_height = RowsPerStrip rows, seg_width == image_width; True: tiles of
                                seg_height x seg_width = TileLength x TileWidth, edge tiles stored at full size
    offsets                     uint32, one per segment, row-major over the segment grid, rebased to the start of the span
    compression                 1: packed samples; 7: every segment is a lossless-JPEG stream
    segments                    compression 7: one _lib.LJPEG_SEG_DTYPE record (mi_ljpeg_seg_t) per segment, its scan_off
                                rebased to the start of the span -- at spp 3 one _lib.LJPEG_SEG3_DTYPE record
                                (mi_ljpeg_seg3_t: streams of three components); else None
    counts                      compression 7: the file's byte count of every segment
    crop_y, crop_x, height, width   the ActiveArea (or the whole image): what comes out
    shift                       every sample is shifted left by it
    table                       the LinearizationTable (uint16) or None
    dtype                       uint8 for 8-bit files, uint16 otherwise
    spp                         samples per pixel (a Python attribute: mi_raw_layout_t does not carry it).  1: a mosaic or a grey
                                frame.  3: a LinearRaw frame -- the layout then describes SAMPLES, not pixels: image_width,
                                seg_width, crop_x and width are the pixel values times 3, which is how chunky rows lie, so
                                raw_unpack decodes them unchanged and its H x 3W samples are the H x W x 3 RGB frame
    """

    def __init__(self, bits, big_endian, image_height, image_width, tiled, seg_height, seg_width, offsets, crop_y=0, crop_x=0,
                 height=None, width=None, shift=0, table=None, compression=1, segments=None, counts=None, spp=1):
        self.spp = int(spp)
        self.bits, self.big_endian = int(bits), bool(big_endian)
        self.image_height, self.image_width = int(image_height), int(image_width)
        self.tiled, self.seg_height, self.seg_width = bool(tiled), int(seg_height), int(seg_width)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        self.crop_y, self.crop_x = int(crop_y), int(crop_x)
        self.height = self.image_height - self.crop_y if height is None else int(height)
        self.width = self.image_width - self.crop_x if width is None else int(width)
        self.shift = int(shift)
        self.table = None if table is None else np.ascontiguousarray(table, dtype=np.uint16)
        self.dtype = np.dtype(np.uint8 if self.bits == 8 else np.uint16)
        self.compression = int(compression)
        seg_dtype = _lib.LJPEG_SEG3_DTYPE if self.spp == 3 else _lib.LJPEG_SEG_DTYPE     # (three tables for three components)
        self.segments = None if segments is None else np.ascontiguousarray(segments, dtype=seg_dtype)
        self.counts = None if counts is None else np.ascontiguousarray(counts, dtype=np.int64)

    def __repr__(self):
        seg = f"tiles {self.seg_height}x{self.seg_width}" if self.tiled else f"strips of {self.seg_height} rows"
        return (f"RawLayout({self.bits} bit{', big-endian' if self.big_endian else ''}{', lossless JPEG' if self.compression == 7 else ''}, "
                f"{self.image_height}x{self.image_width}, {seg}, "
                f"crop ({self.crop_y}, {self.crop_x}) {self.height}x{self.width}, shift {self.shift}, "
                f"table {None if self.table is None else len(self.table)})")

    @property
    def row_bytes(self):
        """bytes of one row of a segment: every row starts on a byte boundary"""
        return (self.seg_width * self.bits + 7) // 8

    @property
    def grid(self):
        """(segments down, segments across)"""
        return -(-self.image_height // self.seg_height), -(-self.image_width // self.seg_width)

    def segment_bytes(self, k):
        """the stored bytes of segment k: a tile is always whole, the last strip holds the rows that are left; of a
        compressed layout the file's byte count"""
        if self.compression == 7:
            return int(self.counts[k])
        return self.segment_rows(k) * self.row_bytes

    def segment_rows(self, k):
        sy = k // self.grid[1]
        return self.seg_height if self.tiled else min(self.seg_height, self.image_height - sy * self.seg_height)

    def struct(self):
        """mi_raw_layout_t"""
        return _lib.RawLayoutStruct(self.bits, int(self.big_endian), self.image_height, self.image_width, int(self.tiled),
                                    self.seg_height, self.seg_width, self.crop_y, self.crop_x, self.height, self.width, self.shift,
                                    0 if self.table is None else len(self.table), _lib.DTYPE_CODE[self.dtype])


class DngFrame:
    """One parsed DNG file (see the module's docstring).  `span` is a read-only view of the file's mapping: the frame keeps
    the mapping alive."""

    def __init__(self, path, layout, span, cfa, develop, lens, orientation, ignored, corrections=None, finish=None, linear=None):
        self.path, self.layout, self.span, self.cfa = path, layout, span, cfa
        self.linear = linear                # a demosaic.Linear for a LinearRaw frame (`cfa` is then None), else None
        self.develop, self.lens, self.orientation, self.ignored = develop, lens, orientation, tuple(ignored)
        self.corrections = corrections      # a SiteCorrections, or None when the file carries none
        self.finish = Finish(orientation=orientation) if finish is None else finish    # the file's own Finish

    def remaining(self, corrections="auto", finish=None):
        """`ignored` minus what `corrections` ("auto": the file's own, None: nothing, or a SiteCorrections) and `finish` ("auto",
        None or a Finish) apply: one entry leaves per applied tag or opcode, and "OpcodeList2" with them when every opcode of
        that list is applied.  (OpcodeList3 itself is never listed: only its opcodes are, and FixVignetteRadial leaves with a
        finish that applies it.)"""
        c = resolve_corrections(self, corrections)
        f = resolve_finish(self, finish)
        left = list(self.ignored)
        for name in (() if c is None else c.applies) + (() if f is None else f.applies):
            if name in left:
                left.remove(name)
        if c is not None and c.whole_list2 and "OpcodeList2" in left:
            left.remove("OpcodeList2")
        return tuple(left)

    def finished_shape(self, finish="auto"):
        """(H', W') of the developed frame under `finish` ("auto": the file's own, None, or a Finish)"""
        f = resolve_finish(self, finish)
        return self.shape if f is None else f.finished_shape(self.shape)

    @property
    def shape(self):
        """(H, W) in pixels"""
        return self.layout.height, self.layout.width // self.layout.spp

    @property
    def dtype(self):
        return self.layout.dtype

    def __repr__(self):
        return f"DngFrame({self.path!r}, {self.layout!r}, {self.cfa if self.linear is None else self.linear!r}, ignored={list(self.ignored)})"


class Raw:
    """How FocusStack, FocusStackBunch, CombinedActions and PyramidStack take `.dng` input (their `raw=` option).

    develop      "auto": each file's own `DngFrame.develop` (its colour matrix and the sRGB curve); None: the plain demosaic;
                 a demosaic.Develop: that one for every file
    lens         "auto": the file's WarpRectilinear opcode; None: no lens correction; a lens.Lens: that one
    calibration  a demosaic.Calibration applied to every unpacked mosaic, or None
    corrections  None: the file's site corrections are not applied (`DngFrame.ignored` lists them); "auto": each file's own
                 `DngFrame.corrections`; a SiteCorrections: that one for every file.  Ahead of `calibration`.
    finish       None: vignette, default crop and orientation of the file are not applied (the frame comes out as stored);
                 "auto": each file's own `DngFrame.finish`; a Finish: that one for every file.  The vignette gain follows
                 the site corrections, crop and orientation are the last stage: the stack, its depth map and everything
                 derived from them come out in the finished geometry.

    ljpeg_split  False: lossless-JPEG files are decoded one segment a wavefront (raw_ljpeg); True, or {"sub_bytes": ...,
                 "max_rounds": ...}: by the split path, which decodes inside a segment (csrc/kernels_ljpeg_split.hpp) -- the
                 same samples, sooner for files in long strips or one strip.  Three-sample LinearRaw files keep going to
                 raw_ljpeg3, silently: the same result.

    LinearRaw files of a folder take the same options where they mean something (develop, lens, finish); `calibration`, a
    `develop` with defect sites and a SiteCorrections object are per CFA site and raise InvalidOptionError at such a file
    (`check_linear_options`), "auto" records what the file carries as skipped.
    """

    def __init__(self, develop="auto", lens="auto", calibration=None, corrections=None, finish=None, ljpeg_split=False):
        from .demosaic import check_calibration, check_develop
        from .lens import check_lens
        if not (isinstance(develop, str) and develop == "auto") and develop is not None:
            check_develop(develop)
        if not (isinstance(lens, str) and lens == "auto") and lens is not None:
            lens = check_lens(lens)
        if calibration is not None:
            check_calibration(calibration)
        if not (isinstance(corrections, str) and corrections == "auto") and corrections is not None:
            check_corrections(corrections)
        if not (isinstance(finish, str) and finish == "auto") and finish is not None:
            check_finish(finish)
        try:
            _lib.ljpeg_split_options(ljpeg_split)
        except (TypeError, ValueError) as e:
            raise InvalidOptionError("ljpeg_split", ljpeg_split, str(e))
        self.develop, self.lens, self.calibration, self.corrections, self.finish = develop, lens, calibration, corrections, finish
        self.ljpeg_split = ljpeg_split if ljpeg_split else False

    def __repr__(self):
        tail = "" if self.corrections is None else f", corrections={self.corrections!r}"
        tail += "" if self.finish is None else f", finish={self.finish!r}"
        tail += "" if not self.ljpeg_split else f", ljpeg_split={self.ljpeg_split!r}"
        return f"Raw(develop={self.develop!r}, lens={self.lens!r}, calibration={self.calibration!r}{tail})"

    def corrections_for(self, frame):
        return frame.corrections if isinstance(self.corrections, str) else self.corrections

    def finish_for(self, frame):
        """the Finish applied to `frame`, or None when there is nothing to apply"""
        return resolve_finish(frame, self.finish)

    def develop_for(self, frame):
        return frame.develop if isinstance(self.develop, str) else self.develop

    def lens_for(self, frame):
        return frame.lens if isinstance(self.lens, str) else self.lens


def check_raw(raw):
    if not isinstance(raw, Raw):
        raise InvalidOptionError("raw", raw, "a shinestacker_amd.dng.Raw is expected")
    return raw


def is_dng(path):
    return str(path).split(".")[-1].lower() in EXTENSIONS


# ---------------------------------------------------------------- site corrections
SITE_MAX_NODES = 4096                           # sitecorr::MAX_NODES of csrc/kernels_sitecorr.hpp: mv, mh of one grid
SITE_GAIN_ONE = 4096                            # Q12
SITE_MAX_BAD = 1 << 20                          # sites a file's bad-pixel list may expand to
SITE_VEC_BYTES = 16                             # sitecorr::VEC_BYTES: one lane's window of a row
SITE_TILE_H, SITE_LANES = 4, 64                 # sitecorr::TILE_H / LANES: a workgroup is 4 rows of 64 windows


def site_vec(dtype):
    """the site-correction kernel's vector width in sites for mosaics of `dtype`"""
    return SITE_VEC_BYTES // np.dtype(dtype).itemsize


def site_tile(dtype):
    """(rows, sites of a row) of one workgroup of the site-correction kernel, for rows that start on a 16-byte boundary"""
    return SITE_TILE_H, SITE_LANES * site_vec(dtype)


def relative(k, n):
    """Row or column k of an n-pixel image in an opcode's relative coordinates (0.0: the image's first edge, 1.0: its last):
    the pixel's centre.  The ONE place the formula stands: pinning the reader against a real DNG changes this line."""
    return (np.asarray(k, np.float64) + 0.5) / float(n)


def _half_up(x):
    return np.floor(np.asarray(x, np.float64) + 0.5)


class GainMap:
    """One gain map: `nodes` (mv x mh float64, each finite and in [0, 16)), `spacing` (vertical, horizontal) and `origin`
    (vertical, horizontal) of the node grid in relative coordinates (`relative`).  Between nodes the gain is bilinear; outside
    the grid the edge node holds."""

    def __init__(self, nodes, spacing=(1.0, 1.0), origin=(0.0, 0.0)):
        n = np.array(nodes, np.float64)
        if n.ndim != 2 or not 1 <= n.shape[0] <= SITE_MAX_NODES or not 1 <= n.shape[1] <= SITE_MAX_NODES:
            raise InvalidOptionError("nodes", n.shape, f"a grid of 1 to {SITE_MAX_NODES} nodes each way is expected")
        if not np.isfinite(n).all() or n.min() < 0.0 or n.max() >= 16.0:
            raise InvalidOptionError("nodes", "values", "every node is finite and lies in [0, 16)")
        sp, og = tuple(float(v) for v in spacing), tuple(float(v) for v in origin)
        if len(sp) != 2 or len(og) != 2 or not all(math.isfinite(v) for v in sp + og) or min(sp) < 0.0:
            raise InvalidOptionError("spacing", (spacing, origin), "two finite numbers each, the spacing not negative")
        self.nodes, self.spacing, self.origin = n, sp, og

    def __repr__(self):
        return f"GainMap({self.nodes.shape[0]} x {self.nodes.shape[1]}, spacing={self.spacing}, origin={self.origin})"

    def nodes_q(self):
        """the nodes in Q12, uint16: round-half-up(node * 4096), at most 65535"""
        return np.minimum(_half_up(self.nodes * float(SITE_GAIN_ONE)), 65535.0).astype(np.uint16)

    @staticmethod
    def axis(n_sites, n_nodes, spacing, origin):
        """one axis entry (node, weight) per row or column: t = (relative(k, n) - origin) / spacing clamped to the grid,
        node = floor(t), weight = round-half-up(256 (t - node)) of the node behind it"""
        out = np.zeros(n_sites, _lib.SITE_AXIS_DTYPE)
        if n_nodes > 1 and spacing > 0.0:
            t = np.clip((relative(np.arange(n_sites), n_sites) - origin) / spacing, 0.0, float(n_nodes - 1))
            i = np.minimum(np.floor(t), n_nodes - 1)
            out["node"] = i.astype(np.uint16)
            out["weight"] = _half_up((t - i) * 256.0).astype(np.uint16)
        return out

    def axes(self, shape):
        """(row axis, column axis) over an H x W image"""
        return (self.axis(int(shape[0]), self.nodes.shape[0], self.spacing[0], self.origin[0]),
                self.axis(int(shape[1]), self.nodes.shape[1], self.spacing[1], self.origin[1]))


class SiteTables:
    """The integer tables the site-correction kernels take (SiteCorrections.quantised): `dh` / `dv` int16 or None, `gains` four
    entries of None or (nodes uint16 mv x mh, row axis, column axis), `bad_sites` int32 ascending, `bad_constant` (value, mask)
    or None."""

    def __init__(self, dh, dv, gains, bad_sites, bad_constant):
        self.dh, self.dv, self.gains, self.bad_sites, self.bad_constant = dh, dv, gains, bad_sites, bad_constant

    @property
    def flags(self):
        return ((_lib.MI_SITE_DELTA_H if self.dh is not None else 0) | (_lib.MI_SITE_DELTA_V if self.dv is not None else 0) |
                (_lib.MI_SITE_GAIN if any(g is not None for g in self.gains) else 0) |
                (_lib.MI_SITE_BAD_LIST if len(self.bad_sites) else 0) | (_lib.MI_SITE_BAD_CONST if self.bad_constant is not None else 0))

    def arrays(self):
        """every table, in a fixed order, each named: what struct() points into"""
        out = []
        if self.dh is not None:
            out.append(("dh", self.dh))
        if self.dv is not None:
            out.append(("dv", self.dv))
        for p, g in enumerate(self.gains):
            if g is not None:
                out += [(f"nodes{p}", g[0]), (f"row{p}", g[1]), (f"col{p}", g[2])]
        if len(self.bad_sites):
            out.append(("bad", self.bad_sites))
        return out

    def same(self, other):
        a, b = self.arrays(), other.arrays()
        return (self.bad_constant == other.bad_constant and [n for n, _ in a] == [n for n, _ in b] and
                all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for (_, x), (_, y) in zip(a, b)))

    def struct(self, address):
        """mi_site_correct_t whose pointers are address(name, array): host addresses, or those of resident copies"""
        c = _lib.SiteCorrectStruct()
        c.flags = self.flags
        if self.dh is not None:
            c.delta_h = address("dh", self.dh)
        if self.dv is not None:
            c.delta_v = address("dv", self.dv)
        for p, g in enumerate(self.gains):
            if g is not None:
                c.gain[p].nodes, c.gain[p].row_axis, c.gain[p].col_axis = (address(f"nodes{p}", g[0]), address(f"row{p}", g[1]),
                                                                           address(f"col{p}", g[2]))
                c.gain[p].mv, c.gain[p].mh = g[0].shape
        if len(self.bad_sites):
            c.bad_sites, c.n_bad = address("bad", self.bad_sites), len(self.bad_sites)
        if self.bad_constant is not None:
            c.bad_constant, c.bad_phase_mask = self.bad_constant
        return c

    def host_struct(self):
        return self.struct(lambda name, a: a.ctypes.data)


class SiteCorrections:
    """The per-site corrections of a raw frame, applied to the unpacked mosaic ahead of everything else (see the module's
    docstring for the order; csrc/kernels_sitecorr.hpp for the arithmetic).

    black_h, black_v   integer arrays of W and H entries in the mosaic's scale, added to the black level per column and per row
                       (a file's BlackLevelDeltaH/V: round-half-up of the delta times 2^shift), or None
    gains              None, one GainMap for every position, or four entries (None or a GainMap) for the positions
                       2 (y & 1) + (x & 1)
    bad_sites          linear indices y * W + x into the cropped mosaic, or an (n, 2) array of (y, x) with `shape`; kept
                       ascending and unique, int32
    bad_constant       (value, mask): every site of the positions in the 4-bit `mask` (bit pos) that holds `value` is repaired
    skipped            a tuple of (name, reason): what a file carried and this object does not apply
    applies            the names, as `DngFrame.ignored` spells them, of what this object applies (None: derived from the above)

    `quantised(shape, dtype)` is the one function that turns geometry into the kernel's axis entries.  The device tables of
    `prepared` are uploaded per device at first use and held until close()."""

    def __init__(self, black_h=None, black_v=None, gains=None, bad_sites=None, bad_constant=None, skipped=(), applies=None,
                 whole_list2=False):
        def delta(name, v):
            if v is None:
                return None
            a = np.asarray(v)
            if a.ndim != 1 or a.dtype.kind not in "iu" or len(a) < 2:
                raise InvalidOptionError(name, getattr(a, "shape", v), "a one-dimensional integer array is expected")
            a = a.astype(np.int64)
            if a.min() < -32768 or a.max() > 32767:
                raise InvalidOptionError(name, (int(a.min()), int(a.max())), "the deltas fit 16 bits")
            return a
        self.black_h, self.black_v = delta("black_h", black_h), delta("black_v", black_v)
        if gains is None:
            self.gains = (None,) * 4
        elif isinstance(gains, GainMap):
            self.gains = (gains,) * 4
        else:
            g = tuple(gains)
            if len(g) != 4 or not all(m is None or isinstance(m, GainMap) for m in g):
                raise InvalidOptionError("gains", gains, "one GainMap, or four entries (a GainMap or None per position)")
            self.gains = g
        self.bad_sites = np.zeros(0, np.int32)
        if bad_sites is not None:
            b = np.asarray(bad_sites)
            if b.size and (b.ndim != 1 or b.dtype.kind not in "iu" or b.min() < 0 or b.max() >= 2 ** 31):
                raise InvalidOptionError("bad_sites", b.shape, "a one-dimensional array of linear indices y * W + x is expected")
            self.bad_sites = np.unique(b.astype(np.int64)).astype(np.int32)
        self.bad_constant = None
        if bad_constant is not None:
            try:
                value, mask = (int(v) for v in bad_constant)
            except (TypeError, ValueError):
                raise InvalidOptionError("bad_constant", bad_constant, "a (value, mask) pair of ints is expected") from None
            if not 0 <= value <= 65535 or not 1 <= mask <= 15:
                raise InvalidOptionError("bad_constant", bad_constant, "the value lies in [0, 65535], the position mask in [1, 15]")
            self.bad_constant = (value, mask)
        self.skipped = tuple((str(n), str(r)) for n, r in skipped)
        if applies is None:
            maps = []
            for m in self.gains:
                if m is not None and not any(m is x for x in maps):
                    maps.append(m)
            applies = ((["BlackLevelDeltaH"] if self.black_h is not None else []) + (["BlackLevelDeltaV"] if self.black_v is not None else []) +
                       (["FixBadPixelsList"] if len(self.bad_sites) else []) + (["FixBadPixelsConstant"] if self.bad_constant else []) +
                       ["GainMap"] * len(maps))
        self.applies, self.whole_list2 = tuple(applies), bool(whole_list2)
        self._quant = {}        # (h, w, dtype) -> SiteTables
        self._dev = {}          # (device, h, w, dtype) -> (mi_site_correct_t, [DeviceBuffer])

    def __repr__(self):
        maps = [None if m is None else f"{m.nodes.shape[0]}x{m.nodes.shape[1]}" for m in self.gains]
        return (f"SiteCorrections(black_h={None if self.black_h is None else len(self.black_h)}, "
                f"black_v={None if self.black_v is None else len(self.black_v)}, gains={maps}, bad_sites={len(self.bad_sites)}, "
                f"bad_constant={self.bad_constant}, skipped={list(self.skipped)})")

    @property
    def empty(self):
        return (self.black_h is None and self.black_v is None and all(m is None for m in self.gains) and len(self.bad_sites) == 0 and
                self.bad_constant is None)

    def quantised(self, shape, dtype):
        """The SiteTables for H x W mosaics of `dtype`: the deltas as int16, every map's nodes in Q12 with one axis entry per
        row and per column (GainMap.axis), the bad sites, the constant.  Checked against the frame: table lengths, sites
        inside it, a constant the dtype holds."""
        h, w = int(shape[0]), int(shape[1])
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            from .errors import BitDepthError
            raise BitDepthError("uint8 or uint16", dt)
        key = (h, w, dt)
        if key not in self._quant:
            if h < 2 or w < 2 or h * w >= 2 ** 31:
                raise InvalidOptionError("shape", (h, w), "a mosaic is H x W with H, W >= 2 and H * W < 2^31")
            if self.black_h is not None and len(self.black_h) != w:
                raise InvalidOptionError("black_h", len(self.black_h), f"a {h} x {w} mosaic has {w} columns")
            if self.black_v is not None and len(self.black_v) != h:
                raise InvalidOptionError("black_v", len(self.black_v), f"a {h} x {w} mosaic has {h} rows")
            if len(self.bad_sites) and int(self.bad_sites[-1]) >= h * w:
                raise InvalidOptionError("bad_sites", int(self.bad_sites[-1]), f"a site lies outside the {h} x {w} mosaic")
            if self.bad_constant is not None and self.bad_constant[0] > int(np.iinfo(dt).max):
                raise InvalidOptionError("bad_constant", self.bad_constant, f"the value exceeds the maximum of {dt}")
            done, gains = [], []
            for m in self.gains:        # positions that share a map share its tables
                hit = next((t for x, t in done if x is m), None)
                if m is not None and hit is None:
                    ra, ca = m.axes((h, w))
                    hit = (np.ascontiguousarray(m.nodes_q()), ra, ca)
                    done.append((m, hit))
                gains.append(hit)
            self._quant[key] = SiteTables(None if self.black_h is None else self.black_h.astype(np.int16),
                                          None if self.black_v is None else self.black_v.astype(np.int16), tuple(gains),
                                          self.bad_sites, self.bad_constant)
        return self._quant[key]

    def prepared(self, shape, dtype, device=0):
        """mi_site_correct_t whose tables are resident on `device` (uploaded at first use, held until close()).  With a
        constant it carries one scratch plane: kernels queued with it on two streams at once would share that plane."""
        q = self.quantised(shape, dtype)
        key = (device, int(shape[0]), int(shape[1]), np.dtype(dtype))
        if key not in self._dev:
            _lib.require_device()
            bufs, seen = [], {}

            def resident(name, a):
                if id(a) not in seen:
                    buf = _lib.DeviceBuffer(a.nbytes, device)
                    buf.upload(a)
                    bufs.append(buf)
                    seen[id(a)] = buf.ptr
                return seen[id(a)]
            sc = q.struct(resident)
            if q.bad_constant is not None:      # the bit plane between the constant repair's two passes
                bufs.append(_lib.DeviceBuffer(8 * (-(-key[1] * key[2] // 64)), device))
                sc.dev_scratch = bufs[-1].ptr
            self._dev[key] = (sc, bufs)
        return self._dev[key][0]

    def close(self):
        """free the device tables (not before every kernel queued with them has run)"""
        for _, bufs in self._dev.values():
            for buf in bufs:
                buf.free()
        self._dev = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_corrections(corrections):
    if not isinstance(corrections, SiteCorrections):
        raise InvalidOptionError("corrections", corrections, '"auto", None or a shinestacker_amd.dng.SiteCorrections is expected')
    return corrections


def resolve_corrections(frame, corrections):
    """None, the frame's own ("auto") or the given SiteCorrections; one that holds nothing counts as None"""
    if isinstance(corrections, str):
        if corrections != "auto":
            raise InvalidOptionError("corrections", corrections, '"auto", None or a dng.SiteCorrections is expected')
        corrections = None if frame is None else frame.corrections
    elif corrections is not None:
        check_corrections(corrections)
    return None if corrections is None or corrections.empty else corrections


def _gain_map(body, h, w):
    """a GainMap opcode's data -> (positions, GainMap), or a str: the reason it is skipped.  Layout: Top, Left, Bottom, Right,
    Plane, Planes, RowPitch, ColPitch, MapPointsV, MapPointsH (uint32), MapSpacingV, MapSpacingH, MapOriginV, MapOriginH
    (double), MapPlanes (uint32) -- 76 bytes -- then MapPointsV x MapPointsH x MapPlanes float32, all big-endian."""
    if len(body) < 76:
        return f"a body of {len(body)} bytes is shorter than its 76-byte header"
    top, left, bottom, right, _plane, planes, rp, cp, mv, mh = struct.unpack(">10I", body[:40])
    sv, sh, ov, oh = struct.unpack(">4d", body[40:72])
    mplanes = struct.unpack(">I", body[72:76])[0]
    if mv == 0 or mh == 0:
        return "zero map points"
    if planes != 1 or mplanes != 1:
        return f"Planes = {planes}, MapPlanes = {mplanes}: one plane is read"
    if mv > SITE_MAX_NODES or mh > SITE_MAX_NODES:
        return f"{mv} x {mh} map points: at most {SITE_MAX_NODES} each way"
    if len(body) < 76 + 4 * mv * mh:
        return f"a body of {len(body)} bytes is shorter than its {mv} x {mh} map points"
    if rp not in (1, 2) or cp not in (1, 2):
        return f"RowPitch = {rp}, ColPitch = {cp}: a pitch of 1 or 2 is read"
    last_y, last_x = (h - 1) - ((h - 1 - top) % rp) if top < h else -1, (w - 1) - ((w - 1 - left) % cp) if left < w else -1
    if top >= rp or left >= cp or bottom <= last_y or right <= last_x:
        return f"the rectangle ({top}, {left}, {bottom}, {right}) does not span the {h} x {w} image"
    if not all(math.isfinite(v) for v in (sv, sh, ov, oh)) or sv < 0.0 or sh < 0.0:
        return "a spacing or origin that is not finite, or a negative spacing"
    nodes = np.array(struct.unpack(f">{mv * mh}f", body[76:76 + 4 * mv * mh]), np.float64).reshape(mv, mh)
    if not np.isfinite(nodes).all():
        return "a map point that is not finite"
    if nodes.min() < 0.0:
        return "a negative map point"
    if nodes.max() >= 16.0:
        return "a map point of 16 or more"
    rows = (0, 1) if rp == 1 else (top & 1,)
    cols = (0, 1) if cp == 1 else (left & 1,)
    return [2 * py + px for py in rows for px in cols], GainMap(nodes, (sv, sh), (ov, oh))


def _bad_list(body, h, w):
    """a FixBadPixelsList opcode's data -> ascending linear indices inside the H x W image, or a str: the reason it is skipped.
    Layout: BayerPhase, BadPointCount, BadRectCount (uint32), the points as (row, column), the rectangles as (top, left,
    bottom, right), all uint32 big-endian."""
    if len(body) < 12:
        return f"a body of {len(body)} bytes is shorter than its 12-byte header"
    _phase, npts, nrect = struct.unpack(">3I", body[:12])
    if len(body) < 12 + 8 * npts + 16 * nrect:
        return f"a body of {len(body)} bytes is shorter than its {npts} points and {nrect} rectangles"
    pts = np.array(struct.unpack(f">{2 * npts}I", body[12:12 + 8 * npts]), np.int64).reshape(npts, 2)
    rects = np.array(struct.unpack(f">{4 * nrect}I", body[12 + 8 * npts:12 + 8 * npts + 16 * nrect]), np.int64).reshape(nrect, 4)
    t, l = np.clip(rects[:, 0], 0, h), np.clip(rects[:, 1], 0, w)
    b, r = np.clip(rects[:, 2], t, h), np.clip(rects[:, 3], l, w)
    total = npts + int((np.maximum(rects[:, 2] - rects[:, 0], 0) * np.maximum(rects[:, 3] - rects[:, 1], 0)).sum())   # as the file states them
    if total > SITE_MAX_BAD:
        return f"the list expands to {total} sites: at most 2^20 are read"
    inside = pts[(pts[:, 0] < h) & (pts[:, 1] < w)]
    sites = [inside[:, 0] * w + inside[:, 1]]
    for k in range(nrect):
        yy, xx = np.mgrid[t[k]:b[k], l[k]:r[k]]
        sites.append((yy * w + xx).reshape(-1))
    return np.unique(np.concatenate(sites)).astype(np.int32)


def _site_corrections(t, rawifd, ifd0, ops2, layout, black, path):
    """the SiteCorrections of a file, or None when it carries none: BlackLevelDeltaH/V of the raw IFD (or IFD0) and the
    GainMap, FixBadPixelsConstant and FixBadPixelsList opcodes `ops2` of OpcodeList2.  black: the four levels, unshifted."""
    if layout.spp != 1 or black is None:
        # a LinearRaw frame has no CFA sites: every per-site correction the file carries is recorded as skipped
        skipped = [(TAG_NAMES[tag], LINEAR_REASON) for tag in (50715, 50716) if tag in rawifd or tag in ifd0]
        skipped += [(OPCODE_NAMES[oid], LINEAR_REASON) for oid, _ in ops2 if oid in (9, 5, 4)]
        return SiteCorrections(skipped=skipped, applies=()) if skipped else None
    h, w, shift = layout.height, layout.width, layout.shift
    maxv = int(np.iinfo(layout.dtype).max)
    skipped, applies, seen = [], [], False
    deltas = {}
    for tag, n in ((50715, w), (50716, h)):
        c = rawifd if tag in rawifd else ifd0 if tag in ifd0 else None
        if c is None:
            continue
        seen = True
        vals = np.array(t.take(c, tag, 0), np.float64)
        if h < 2 or w < 2:
            skipped.append((TAG_NAMES[tag], f"a crop of {h} x {w}: a mosaic has two rows and two columns at least"))
            continue
        if len(vals) != n:
            skipped.append((TAG_NAMES[tag], f"{len(vals)} entries for a crop of {n} {'columns' if tag == 50715 else 'rows'}"))
            continue
        if not np.isfinite(vals).all() or np.abs(vals).max() * (1 << shift) > 32767:
            skipped.append((TAG_NAMES[tag], "a delta that does not fit 16 bits in the mosaic's scale"))
            continue
        deltas[tag] = _half_up(vals * float(1 << shift)).astype(np.int64)
    if deltas:
        dh, dv = deltas.get(50715, np.zeros(w, np.int64)), deltas.get(50716, np.zeros(h, np.int64))
        for pos in range(4):
            lo = (black[pos] << shift) + dh[pos & 1::2].min() + dv[pos >> 1::2].min()
            hi = (black[pos] << shift) + dh[pos & 1::2].max() + dv[pos >> 1::2].max()
            if lo < 0 or hi > maxv:
                for tag in sorted(deltas):
                    skipped.append((TAG_NAMES[tag], f"black level plus deltas spans {lo} .. {hi} at position {pos}: outside [0, {maxv}]"))
                deltas = {}
                break
    applies += [TAG_NAMES[tag] for tag in sorted(deltas)]
    gains, bad, const, applied2 = [None] * 4, [], None, 0
    for oid, body in ops2:
        name = OPCODE_NAMES.get(oid)
        if oid == 9:
            seen = True
            got = _gain_map(body, h, w)
            if not isinstance(got, str) and any(gains[p] is not None for p in got[0]):
                got = f"a second map for position {next(p for p in got[0] if gains[p] is not None)}"
            if isinstance(got, str):
                skipped.append((name, got))
                continue
            for p in got[0]:
                gains[p] = got[1]
        elif oid == 5:
            seen = True
            got = _bad_list(body, h, w)
            if isinstance(got, str):
                skipped.append((name, got))
                continue
            bad.append(got)
        elif oid == 4:
            seen = True
            if len(body) < 8:
                skipped.append((name, f"a body of {len(body)} bytes is shorter than its 8"))
                continue
            value = struct.unpack(">I", body[:4])[0]
            if layout.table is not None:
                skipped.append((name, "the file has a LinearizationTable: the constant is a stored value, the mosaic holds table entries"))
                continue
            if const is not None:
                skipped.append((name, "a second constant"))
                continue
            if (value << shift) > maxv:
                skipped.append((name, f"the constant {value} lies outside the samples' range"))
                continue
            const = (value << shift, 15)
        else:
            continue
        applies.append(name)
        applied2 += 1
    if not seen:
        return None
    sites = np.unique(np.concatenate(bad)) if bad else None
    return SiteCorrections(deltas.get(50715), deltas.get(50716), gains if any(g is not None for g in gains) else None, sites, const,
                           skipped=skipped, applies=applies, whole_list2=len(ops2) > 0 and applied2 == len(ops2))


# ---------------------------------------------------------------- finish: vignette, crop, orientation
RADIAL_NODES = _lib.RADIAL_NODES                # finish::NODES of csrc/kernels_finish.hpp: u = i / 1024
RADIAL_D2_MAX = 1 << 40                         # finish::D2_MAX
RADIAL_CENTRE_MAX = 1 << 24                     # finish::CENTRE_MAX, half pixels
_INVERT_SAMPLES = 1 << 16                       # intervals of [0, 1] over which a warp's radial map is inverted


def radial_d2max(h, w, cx2, cy2):
    """the largest d2 = (2x - cx2)^2 + (2y - cy2)^2 of the four corner sites of an H x W mosaic: what the kernel's radius is
    normalised by"""
    return max((2 * x - cx2) ** 2 + (2 * y - cy2) ** 2 for x in (0, w - 1) for y in (0, h - 1))


class RadialGain:
    """A radial gain on the linear mosaic: g(u) = 1 + k0 u + k1 u^2 + k2 u^3 + k3 u^4 + k4 u^5 with u = r^2, r the distance
    from `centre` normalised to 1 at the farthest corner site, as lens.Lens normalises its radius (a DNG's
    FixVignetteRadial: 1 + k0 r^2 + ... + k4 r^10).

    k           (k0, k1, k2, k3, k4), finite, with 0 < g < 16 on [0, 1]
    centre      (cx, cy) in pixels; the kernel takes it rounded to half pixels
    after_warp  the polynomial is stated in the lens-corrected frame (the opcode stands behind a WarpRectilinear).  The
                gain is applied to the mosaic, ahead of the lens remap, so when a lens IS applied the table is built over
                the SOURCE radius: table(u_src) = g(u_dst(u_src)), where u_src = u_dst s(u_dst)^2 is GREEN's radial map
                (lens.Lens, destination -> source, about the same centre), inverted numerically in float64.  A map that is
                not strictly increasing on [0, 1] is refused.  Red and blue have their own magnifications (lateral CA) and
                get green's table: the differing CA magnifications are IGNORED here.  A plane whose own map puts a site at
                u_dst + du gets the gain of u_dst, off by at most max|g'| du: for the tests' polynomial (0.3, 0.1, 0, 0, 0),
                max|g'| = 0.5, under planes of 1.01 / 1.0 / 0.99 (the largest CA the tests write) du <= 0.0204 and the
                gain error is at most 0.0102, one percent of the gain (tests/test_finish_host.py computes both)."""

    def __init__(self, k, centre, after_warp=False):
        try:
            kk = tuple(float(v) for v in k)
            c = tuple(float(v) for v in centre)
        except (TypeError, ValueError):
            raise InvalidOptionError("vignette", (k, centre), "five numbers (k0..k4) and a centre (cx, cy) are expected") from None
        if len(kk) != 5 or len(c) != 2:
            raise InvalidOptionError("vignette", (k, centre), "five numbers (k0..k4) and a centre (cx, cy) are expected")
        if not all(math.isfinite(v) for v in kk + c):
            raise InvalidOptionError("vignette", (k, centre), "the coefficients and the centre must be finite")
        if max(abs(v) for v in c) > RADIAL_CENTRE_MAX // 2:
            raise InvalidOptionError("vignette", centre, "the centre lies at most 2^23 pixels from the origin")
        self.k, self.centre, self.after_warp = kk, c, bool(after_warp)
        lo, hi = self.range()
        if not lo > 0.0 or not hi < 16.0:
            raise InvalidOptionError("vignette", k, f"the gain spans {lo} .. {hi} on [0, 1]: it must stay inside (0, 16)")
        self._dev = {}          # (device, lens key) -> DeviceBuffer of the table

    def __repr__(self):
        return f"RadialGain(k={list(self.k)}, centre={self.centre}{', after_warp=True' if self.after_warp else ''})"

    def gain(self, u):
        """g(u), float64"""
        u = np.asarray(u, np.float64)
        k0, k1, k2, k3, k4 = self.k
        return 1.0 + u * (k0 + u * (k1 + u * (k2 + u * (k3 + u * k4))))

    def range(self):
        """(min, max) of g over 4097 points of [0, 1]"""
        g = self.gain(np.linspace(0.0, 1.0, 4097))
        return float(g.min()), float(g.max())

    def centre2(self):
        """the centre in half pixels: round-half-up(2 cx), round-half-up(2 cy)"""
        return int(_half_up(2.0 * self.centre[0])), int(_half_up(2.0 * self.centre[1]))

    @staticmethod
    def source_map(lens):
        """(u_dst, u_src) over [0, 1]: green's radial map u_src = u_dst s(u_dst)^2 on _INVERT_SAMPLES intervals; raises
        InvalidOptionError when it is not strictly increasing"""
        from .lens import check_lens
        k0, k1, k2, k3 = check_lens(lens).k[1]
        ud = np.linspace(0.0, 1.0, _INVERT_SAMPLES + 1)
        s = ((k3 * ud + k2) * ud + k1) * ud + k0
        us = ud * s * s
        if not (s > 0.0).all() or not (np.diff(us) > 0.0).all():
            raise InvalidOptionError("lens", lens, "green's radial map is not monotone on [0, 1]: the vignette cannot be moved in front of it")
        return ud, us

    def table(self, lens=None):
        """the RADIAL_NODES Q12 uint16 nodes at u = i / 1024: round-half-up(4096 g(u)), at most 65535.  `lens`: the lens.Lens
        applied behind the gain, or None; it matters only with `after_warp` (see the class)."""
        u = np.arange(RADIAL_NODES, dtype=np.float64) / float(RADIAL_NODES - 1)
        if lens is not None and self.after_warp:
            ud, us = self.source_map(lens)
            u = np.interp(u, us, ud)        # (a source radius whose destination lies outside the frame takes the corner's gain)
        return np.minimum(_half_up(self.gain(u) * float(SITE_GAIN_ONE)), 65535.0).astype(np.uint16)

    def check_shape(self, shape):
        """the centre against an H x W mosaic: the farthest corner within the kernel's range"""
        h, w = int(shape[0]), int(shape[1])
        cx2, cy2 = self.centre2()
        d = radial_d2max(h, w, cx2, cy2)
        if not 1 <= d < RADIAL_D2_MAX:
            raise InvalidOptionError("vignette", self.centre, f"the farthest corner of a {h} x {w} mosaic lies {d} half pixels squared away (1 to 2^40 - 1)")
        return cx2, cy2

    def struct(self, shape, lens=None):
        """(mi_radial_gain_t over host memory, the table it points into)"""
        cx2, cy2 = self.check_shape(shape)
        t = np.ascontiguousarray(self.table(lens))
        return _lib.RadialGainStruct(cx2, cy2, t.ctypes.data), t

    def prepared(self, shape, device=0, lens=None):
        """mi_radial_gain_t whose table is resident on `device` (uploaded at first use, held until close())"""
        cx2, cy2 = self.check_shape(shape)
        from .lens import check_lens
        key = (device, None if lens is None or not self.after_warp else check_lens(lens).k[1])
        if key not in self._dev:
            _lib.require_device()
            t = np.ascontiguousarray(self.table(lens))
            buf = _lib.DeviceBuffer(t.nbytes, device)
            buf.upload(t)
            self._dev[key] = buf
        return _lib.RadialGainStruct(cx2, cy2, self._dev[key].ptr)

    def close(self):
        """free the device tables (not before every kernel queued with them has run)"""
        for buf in self._dev.values():
            buf.free()
        self._dev = {}


class Finish:
    """What a raw file says about the finished picture (csrc/kernels_finish.hpp; tests/finish_restatement.py is the definition):

    vignette     None or a RadialGain, applied to the linear mosaic behind the site corrections and ahead of the calibration
                 -- not to the developed frame: Develop's tone curve is not linear, a gain behind it would be wrong
    crop         None or (y, x, h, w) in the coordinates of the unpacked mosaic (a DNG's DefaultCropOrigin / DefaultCropSize)
    orientation  the TIFF orientation 1..8, applied to the cropped frame:  1: a  2: a[:, ::-1]  3: a[::-1, ::-1]  4: a[::-1]
                 5: a.transpose(1, 0, 2)  6: np.rot90(a, -1)  7: a[::-1, ::-1].transpose(1, 0, 2)  8: np.rot90(a, 1)
    skipped      a tuple of (name, reason): what a file carried and this object does not apply
    applies      the names, as `DngFrame.ignored` spells them, of what this object applies (None: derived from the above)

    Crop and orientation are the LAST stage, behind the lens correction: one out-of-place pass over the developed frame."""

    def __init__(self, vignette=None, crop=None, orientation=1, skipped=(), applies=None):
        if vignette is not None and not isinstance(vignette, RadialGain):
            raise InvalidOptionError("vignette", vignette, "None or a shinestacker_amd.dng.RadialGain is expected")
        if crop is not None:
            try:
                c = tuple(crop)
            except TypeError:
                c = ()
            if len(c) != 4 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in c):
                raise InvalidOptionError("crop", crop, "None or four ints (y, x, h, w) are expected")
            crop = tuple(int(v) for v in c)
            if crop[0] < 0 or crop[1] < 0 or crop[2] < 1 or crop[3] < 1:
                raise InvalidOptionError("crop", crop, "the origin is not negative and the size at least 1 x 1")
        if isinstance(orientation, bool) or not isinstance(orientation, (int, np.integer)) or not 1 <= orientation <= 8:
            raise InvalidOptionError("orientation", orientation, "a TIFF orientation 1 to 8 is expected")
        self.vignette, self.crop, self.orientation = vignette, crop, int(orientation)
        self.skipped = tuple((str(n), str(r)) for n, r in skipped)
        if applies is None:
            applies = (["FixVignetteRadial"] if vignette is not None else []) + (["DefaultCropOrigin", "DefaultCropSize"] if crop is not None else [])
        self.applies = tuple(applies)

    def __repr__(self):
        return f"Finish(vignette={self.vignette!r}, crop={self.crop}, orientation={self.orientation}, skipped={list(self.skipped)})"

    @property
    def empty(self):
        return self.vignette is None and self.crop is None and self.orientation == 1

    def crop_for(self, shape):
        """(y, x, h, w) on an H x W frame: the crop checked against it, or the whole frame"""
        h, w = int(shape[0]), int(shape[1])
        if self.crop is None:
            return 0, 0, h, w
        y, x, ch, cw = self.crop
        if y + ch > h or x + cw > w:
            raise InvalidOptionError("crop", self.crop, f"it lies outside the {h} x {w} frame")
        return self.crop

    def geometry(self, shape):
        """True when crop and orientation change an H x W frame at all"""
        return self.orientation != 1 or self.crop_for(shape) != (0, 0, int(shape[0]), int(shape[1]))

    def finished_shape(self, shape):
        """(H', W') of an H x W frame behind crop and orientation"""
        _, _, ch, cw = self.crop_for(shape)
        return (cw, ch) if self.orientation >= 5 else (ch, cw)

    def close(self):
        if self.vignette is not None:
            self.vignette.close()


def check_finish(finish):
    if not isinstance(finish, Finish):
        raise InvalidOptionError("finish", finish, '"auto", None or a shinestacker_amd.dng.Finish is expected')
    return finish


def resolve_finish(frame, finish):
    """None, the frame's own ("auto") or the given Finish; one that holds nothing counts as None"""
    if isinstance(finish, str):
        if finish != "auto":
            raise InvalidOptionError("finish", finish, '"auto", None or a dng.Finish is expected')
        finish = None if frame is None else frame.finish
    elif finish is not None:
        check_finish(finish)
    return None if finish is None or finish.empty else finish


def _fix_vignette_radial(body, h, w):
    """a FixVignetteRadial opcode's data -- seven big-endian doubles k0..k4, cx, cy, the centre in [0, 1] of the image placed as
    `_warp_rectilinear` places its own -- as a RadialGain, or a str: the reason it is skipped"""
    if len(body) < 56:
        return f"a body of {len(body)} bytes is shorter than its seven doubles"
    vals = struct.unpack(">7d", body[:56])
    if not all(math.isfinite(v) for v in vals):
        return "a coefficient or the centre is not finite"
    try:
        return RadialGain(vals[:5], (vals[5] * (w - 1), vals[6] * (h - 1)))
    except InvalidOptionError as exc:
        return str(exc)


def _file_finish(t, rawifd, ifd0, ops3, shape, lens, orientation, linear=False):
    """the Finish of a file whose frame is `shape` = (H, W) pixels: FixVignetteRadial of OpcodeList3 (`ops3`), DefaultCropOrigin /
    DefaultCropSize, Orientation.  `linear`: a LinearRaw file -- its FixVignetteRadial is skipped (the radial-gain kernel
    addresses mosaic sites)."""
    h, w = shape
    skipped = []

    def get(tag):
        for c in (rawifd, ifd0):
            if tag in c:
                return t.take(c, tag, 0)
        return None

    vignette = None
    where = [i for i, (oid, _) in enumerate(ops3) if oid == 3]
    warps = [i for i, (oid, _) in enumerate(ops3) if oid == 1]
    if where and linear:
        skipped.append((OPCODE_NAMES[3], LINEAR_REASON))
    elif where:
        name = OPCODE_NAMES[3]
        scale = get(50718)
        got = _fix_vignette_radial(ops3[where[0]][1], h, w)
        if len(where) > 1:
            got = "a second FixVignetteRadial is present"
        elif scale is not None and any(float(v) != 1.0 for v in scale):
            got = f"the file has DefaultScale = {tuple(scale)}: the radius is stated for the scaled frame"
        elif not isinstance(got, str) and any(i > where[0] for i in warps):
            got = "it stands before the WarpRectilinear: the gain is stated for a frame this reader never holds"
        elif not isinstance(got, str) and warps:
            got.after_warp = True
            if lens is not None:
                lc = lens.resolved_centre(h, w)
                if max(abs(lc[0] - got.centre[0]), abs(lc[1] - got.centre[1])) > 0.5:
                    got = f"its centre {got.centre} is not the WarpRectilinear's {lc}: the warp is inverted about one centre"
                else:
                    try:
                        got.source_map(lens)
                    except InvalidOptionError:
                        got = "the WarpRectilinear's radial map is not monotone on [0, 1]: the gain cannot be moved in front of it"
        if not isinstance(got, str):
            try:
                got.check_shape((h, w))
            except InvalidOptionError as exc:
                got = str(exc)
        if isinstance(got, str):
            skipped.append((name, got))
        else:
            vignette = got
    crop = None
    origin, size = get(50719), get(50720)
    if size is not None or origin is not None:
        names = [TAG_NAMES[tag] for tag, v in ((50719, origin), (50720, size)) if v is not None]
        why = None
        if size is None:
            why = "DefaultCropOrigin without a DefaultCropSize"
        else:
            origin = (0, 0) if origin is None else origin
            vals = [float(v) for v in tuple(origin) + tuple(size)]
            if len(origin) != 2 or len(size) != 2:
                why = f"{len(origin)} and {len(size)} values: two each (horizontal, vertical) are expected"
            elif not all(math.isfinite(v) and v == math.floor(v) for v in vals):
                why = f"origin {tuple(origin)}, size {tuple(size)}: a value that is not integral"
            else:
                x, y, cw, ch = (int(v) for v in vals)
                if x < 0 or y < 0 or cw < 1 or ch < 1 or x + cw > w or y + ch > h:
                    why = f"the rectangle (x {x}, y {y}, {cw} x {ch}) lies outside the {h} x {w} frame"
                else:
                    crop = (y, x, ch, cw)
        if why is not None:
            skipped += [(n, why) for n in names]
    applies = ([OPCODE_NAMES[3]] if vignette is not None else []) + ([TAG_NAMES[tag] for tag, v in ((50719, get(50719)), (50720, size)) if v is not None]
                                                                   if crop is not None else [])
    return Finish(vignette, crop, orientation, skipped=skipped, applies=applies)


# ---------------------------------------------------------------- the TIFF structure
class _Tiff:
    def __init__(self, path, data):
        self.path, self.data = path, data
        head = bytes(data[:8])
        if len(head) < 8 or head[:2] not in (b"II", b"MM"):
            raise ImageLoadError(path, "not a TIFF (no II / MM byte-order mark)")
        self.e = "<" if head[:2] == b"II" else ">"
        if struct.unpack(self.e + "H", head[2:4])[0] != 42:
            raise ImageLoadError(path, "not a TIFF (the magic number is not 42)")
        self.first = struct.unpack(self.e + "I", head[4:8])[0]

    def bytes_at(self, off, n):
        if off < 0 or off + n > len(self.data):
            raise ImageLoadError(self.path, f"truncated: {n} bytes at offset {off} lie outside the {len(self.data)}-byte file")
        return bytes(self.data[off:off + n])

    def ifd(self, off):
        """{tag: (type, count, where the value's bytes lie)} and the offset of the next IFD"""
        n = struct.unpack(self.e + "H", self.bytes_at(off, 2))[0]
        tags = {}
        for i in range(n):
            at = off + 2 + 12 * i
            tag, typ, cnt = struct.unpack(self.e + "HHI", self.bytes_at(at, 8))
            if typ not in _TYPES:
                continue
            nbytes = _TYPES[typ][1] * cnt
            tags[tag] = (typ, cnt, at + 8 if nbytes <= 4 else struct.unpack(self.e + "I", self.bytes_at(at + 8, 4))[0])
        return tags, struct.unpack(self.e + "I", self.bytes_at(off + 2 + 12 * n, 4))[0]

    def raw(self, entry):
        typ, cnt, at = entry
        return self.bytes_at(at, _TYPES[typ][1] * cnt)

    def values(self, entry):
        """the entry's values: ints, floats (RATIONAL and SRATIONAL as numerator / denominator), or bytes for ASCII"""
        typ, cnt, _ = entry
        raw = self.raw(entry)
        if typ == 2:
            return raw
        fmt = _TYPES[typ][0]
        vals = struct.unpack(self.e + fmt * cnt, raw)
        if typ in (5, 10):
            return tuple(vals[2 * i] / vals[2 * i + 1] if vals[2 * i + 1] else 0.0 for i in range(cnt))
        return vals

    def take(self, tags, tag, least=1, integral=False, finite=False):
        """The values of `tag` in the IFD `tags`, as a tuple: at least `least` of them, of an integer type when `integral`,
        FLOAT and DOUBLE values finite when `finite`.  The entry comes from the file: one with fewer values than the reader
        takes, of a type it cannot read as asked or (`finite`) with a NaN in it is an ImageLoadError that names the tag --
        never an IndexError three calls on.  (The corrections a file carries pass neither: what is wrong with one of them
        is a reason to skip it, `skipped`, not to refuse the file.)"""
        typ, cnt, _ = tags[tag]
        name = TAG_NAMES.get(tag, f"tag {tag}")
        if cnt < least:
            raise ImageLoadError(self.path, f"{name} holds {cnt} value{'' if cnt == 1 else 's'} where {least} {'is' if least == 1 else 'are'} read")
        if integral and typ not in _INTEGRAL:
            raise ImageLoadError(self.path, f"{name} has the TIFF type {typ} where an integer type is read")
        vals = tuple(self.values(tags[tag]))
        if finite and typ in (11, 12) and not all(math.isfinite(v) for v in vals):
            raise ImageLoadError(self.path, f"{name} holds a value that is not finite")
        return vals


def _one(t, tags, tag, default):
    """the first value of an integer tag, or `default` when the IFD does not hold it"""
    return t.take(tags, tag, 1, integral=True)[0] if tag in tags else default


def _opcodes(blob, name, path):
    """[(id, data)] of an opcode list: always big-endian -- uint32 count, then per opcode id, version, flags, byte count, data"""
    if len(blob) < 4:
        raise ImageLoadError(path, f"{name} is shorter than its count")
    n = struct.unpack(">I", blob[:4])[0]
    out, at = [], 4
    for _ in range(n):
        if at + 16 > len(blob):
            raise ImageLoadError(path, f"{name} is truncated at opcode {len(out)}")
        oid, _ver, _flags, nb = struct.unpack(">IIII", blob[at:at + 16])
        if at + 16 + nb > len(blob):
            raise ImageLoadError(path, f"{name} is truncated inside opcode {len(out)}")
        out.append((oid, blob[at + 16:at + 16 + nb]))
        at += 16 + nb
    return out


def colour_matrix(color_matrix):
    """camera RGB -> linear sRGB from a DNG ColorMatrix (XYZ -> camera), dcraw's construction:
    cam_from_srgb = ColorMatrix @ XYZ_from_sRGB, every row divided by its sum (camera white maps to sRGB white), inverted."""
    cm = np.asarray(color_matrix, np.float64).reshape(3, 3)
    cam = cm @ XYZ_FROM_SRGB
    cam = cam / cam.sum(axis=1, keepdims=True)
    return np.linalg.inv(cam)


def permute_pattern(pattern, crop_y, crop_x):
    """the 2 x 2 pattern seen from a crop origin: rows swap when crop_y is odd, columns when crop_x is odd"""
    cell = [[pattern[0], pattern[1]], [pattern[2], pattern[3]]]
    return "".join(cell[(py + crop_y) & 1][(px + crop_x) & 1] for py in range(2) for px in range(2))


def read(path):
    """Parse the DNG at `path` into a DngFrame.  TIFF structure only: the sample data is mapped (np.memmap, read-only), not
    read.  The raw IFD is the one with PhotometricInterpretation 32803 (CFA) and NewSubFileType 0, IFD0 or one of its
    SubIFDs; colour tags are looked up in the raw IFD first and in IFD0 after it.

    The colour matrix is the ColorMatrix whose CalibrationIlluminant is 21 (D65), else ColorMatrix2, else ColorMatrix1: the
    two matrices are NOT interpolated between their illuminants.

    What the file says and this reader does not take is refused with InvalidOptionError (the tag's name and value), a file
    that is damaged with ImageLoadError; both messages name the file."""
    path = os.fspath(path)
    try:
        return _read(path)
    except InvalidOptionError as exc:       # (raised by tag and value all over the parse: the file's name goes on here)
        if path in str(exc):
            raise
        raise InvalidOptionError(exc.option, exc.value, f"{exc.details} (in {path})" if exc.details else f"in {path}") from exc


def _read(path):
    if not os.path.isfile(path):
        raise RuntimeError("File does not exist: " + path)
    if os.path.getsize(path) < 8:
        raise ImageLoadError(path, "not a TIFF (shorter than its header)")
    data = np.memmap(path, dtype=np.uint8, mode="r")
    t = _Tiff(path, data)
    ifd0, _ = t.ifd(t.first)
    subs = t.take(ifd0, 330, 0, integral=True) if 330 in ifd0 else ()
    if len(subs) > MAX_SUB_IFDS:    # (each is walked entry by entry: a damaged count must not turn a large file into hours)
        raise ImageLoadError(path, f"SubIFDs holds {len(subs)} offsets (at most {MAX_SUB_IFDS} are followed)")
    cands = [ifd0] + [t.ifd(off)[0] for off in subs]
    rawifd = next((c for c in cands if _one(t, c, 262, None) == CFA_PHOTOMETRIC and _one(t, c, 254, 0) == 0), None)
    linear = rawifd is None
    if linear:      # no mosaic: an already demosaiced frame?
        rawifd = next((c for c in cands if _one(t, c, 262, None) == LINEAR_PHOTOMETRIC and _one(t, c, 254, 0) == 0), None)
    if rawifd is None:
        raise ImageLoadError(path, "no CFA IFD: no IFD with PhotometricInterpretation 32803 and NewSubFileType 0")
    ifd_name = "LinearRaw" if linear else "CFA"

    def get(tag, default=None, integral=False):
        for c in (rawifd, ifd0):
            if tag in c:
                return t.take(c, tag, 1, integral, finite=True)
        return default

    comp = _one(t, rawifd, 259, 1)
    if comp not in (1, 7):
        kind = COMPRESSION_NAMES.get(comp)
        raise InvalidOptionError("Compression", comp, ("compressed samples are not read" if kind is None else
                                                       f"{kind} compressed samples are not read") + ": only uncompressed DNGs")
    spp = _one(t, rawifd, 277, 1)
    if linear and spp not in (1, 3):
        raise InvalidOptionError("SamplesPerPixel", spp, "a LinearRaw frame of 1 or 3 samples per pixel is read")
    if not linear and spp != 1:
        raise InvalidOptionError("SamplesPerPixel", spp, "a CFA mosaic has one sample per pixel")
    bits = _one(t, rawifd, 258, 1)
    if linear:
        every = t.take(rawifd, 258, 1, integral=True) if 258 in rawifd else (1,)
        if len(every) not in (1, spp) or any(b != every[0] for b in every):
            raise InvalidOptionError("BitsPerSample", every, f"one bit depth, or {spp} equal ones, is read")
        planar = _one(t, rawifd, 284, 1)
        if planar != 1:
            raise InvalidOptionError("PlanarConfiguration", planar, "only chunky storage (1) is read: the samples of a pixel lie together")
    if bits not in BITS:
        raise InvalidOptionError("BitsPerSample", bits, "valid values are " + ", ".join(map(str, BITS)))
    if not linear:
        rep = t.take(rawifd, 33421, 1, integral=True) if 33421 in rawifd else (2, 2)
        if rep != (2, 2):
            raise InvalidOptionError("CFARepeatPatternDim", rep, "only 2 x 2 Bayer patterns are read")
        lay = _one(t, rawifd, 50711, 1)
        if lay != 1:
            raise InvalidOptionError("CFALayout", lay, "only the rectangular layout 1 is read")
        planes = tuple(get(50710, (0, 1, 2), integral=True))
        if planes != (0, 1, 2):
            raise InvalidOptionError("CFAPlaneColor", planes, "only red, green, blue (0, 1, 2) is read")
        if 33422 not in rawifd:
            raise ImageLoadError(path, "the CFA IFD has no CFAPattern")
        pat = t.take(rawifd, 33422, 1, integral=True)
        pattern = "".join("RGB"[v] if 0 <= v <= 2 else "?" for v in pat)
        if pattern not in PATTERNS:
            raise InvalidOptionError("CFAPattern", pat, "valid patterns are " + ", ".join(PATTERNS) + " with 0 = R, 1 = G, 2 = B")
    if 256 not in rawifd or 257 not in rawifd:
        raise ImageLoadError(path, f"the {ifd_name} IFD has no ImageWidth / ImageLength")
    iw, ih = _one(t, rawifd, 256, 0), _one(t, rawifd, 257, 0)
    if iw < 1 or ih < 1:
        raise InvalidOptionError("ImageWidth", (iw, ih), "the stored image is empty")
    pw = iw                 # the stored width in pixels; from here iw, sw and the crop count SAMPLES (RawLayout.spp)
    iw *= spp
    dt = np.dtype(np.uint8 if bits == 8 else np.uint16)
    maxv = int(np.iinfo(dt).max)

    # segments
    tiled = 324 in rawifd
    if tiled:
        sw, sh = _one(t, rawifd, 322, 0), _one(t, rawifd, 323, 0)
        if sw < 1 or sh < 1:
            raise InvalidOptionError("TileWidth", (sw, sh), "TileOffsets without a tile size")
        sw *= spp
        off_tag, cnt_tag = 324, 325
    else:
        if 273 not in rawifd:
            raise ImageLoadError(path, f"the {ifd_name} IFD has neither StripOffsets nor TileOffsets")
        sw, sh = iw, min(_one(t, rawifd, 278, ih), ih)
        if sh < 1:
            raise InvalidOptionError("RowsPerStrip", sh, "a strip has at least one row")
        off_tag, cnt_tag = 273, 279
    offs = np.array(t.take(rawifd, off_tag, 1, integral=True), np.int64)
    layout = RawLayout(bits, t.e == ">", ih, iw, tiled, sh, sw, np.zeros(0, np.uint32), compression=comp, spp=spp)
    nseg = layout.grid[0] * layout.grid[1]
    if len(offs) != nseg:
        raise InvalidOptionError(TAG_NAMES[off_tag], len(offs), f"{nseg} segments are expected for a {ih} x {pw} image")
    if comp == 7:
        if cnt_tag not in rawifd:
            raise InvalidOptionError("Compression", 7, f"lossless JPEG: {TAG_NAMES[cnt_tag]} is missing: the length of a compressed "
                                                       "segment is only known from it")
        cnts = np.array(t.take(rawifd, cnt_tag, 1, integral=True), np.int64)
        if len(cnts) != nseg:
            raise InvalidOptionError("Compression", 7, f"lossless JPEG: {TAG_NAMES[cnt_tag]} has {len(cnts)} entries for {nseg} segments")
        layout.counts = cnts
    need = np.array([layout.segment_bytes(k) for k in range(nseg)], np.int64)
    if comp == 7:
        bad = np.flatnonzero((need < 1) | ((offs + need) > len(data)))
        if len(bad):
            k = int(bad[0])
            raise InvalidOptionError("Compression", 7, f"lossless JPEG: segment {k} ({TAG_NAMES[off_tag]}[{k}] = {offs[k]}, {need[k]} bytes) ends "
                                                       f"outside the {len(data)}-byte file")
    elif cnt_tag in rawifd:
        cnts = np.array(t.take(rawifd, cnt_tag, 1, integral=True), np.int64)
        if len(cnts) != nseg or (cnts < need).any():
            k = 0 if len(cnts) != nseg else int(np.flatnonzero(cnts < need)[0])
            raise ImageLoadError(path, f"truncated segment: {TAG_NAMES[cnt_tag]}[{k}] = {cnts[k] if k < len(cnts) else None}, "
                                       f"{need[k]} bytes are needed")
    if ((offs + need) > len(data)).any():
        k = int(np.flatnonzero((offs + need) > len(data))[0])
        raise ImageLoadError(path, f"truncated segment: {TAG_NAMES[off_tag]}[{k}] = {offs[k]} with {need[k]} bytes ends outside the "
                                   f"{len(data)}-byte file")
    lo, hi = int(offs.min()), int((offs + need).max())
    if hi - lo >= 2 ** 32:
        raise InvalidOptionError(TAG_NAMES[off_tag], hi - lo, "the segments span 2^32 bytes or more")
    layout.offsets = (offs - lo).astype(np.uint32)
    span = data[lo:hi]
    if comp == 7:
        # (three samples per pixel: streams of Nf = 3, descriptors with three tables; anything else in the two-table form)
        layout.segments = np.zeros(nseg, _lib.LJPEG_SEG3_DTYPE if spp == 3 else _lib.LJPEG_SEG_DTYPE)
        for k in range(nseg):
            _ljpeg_segment(layout.segments[k:k + 1], k, span, int(layout.offsets[k]), int(need[k]), bits, layout.segment_rows(k), sw,
                           (3,) if spp == 3 else (1, 2))

    # crop
    if 50829 in rawifd:
        area = t.take(rawifd, 50829, 4, integral=True)
        if len(area) != 4:
            raise ImageLoadError(path, f"ActiveArea holds {len(area)} values where 4 are read")
        top, left, bottom, right = (int(v) for v in area)
        if not (0 <= top < bottom <= ih and 0 <= left < right <= pw):
            raise InvalidOptionError("ActiveArea", (top, left, bottom, right), f"it lies outside the {ih} x {pw} image")
        layout.crop_y, layout.crop_x, layout.height, layout.width = top, left * spp, bottom - top, (right - left) * spp

    # levels
    whites = [int(round(v)) for v in get(50717, ((1 << bits) - 1,))]
    if linear and len(whites) not in (1, spp):
        raise InvalidOptionError("WhiteLevel", tuple(whites), f"one value, or one per sample ({spp}), is expected")
    whites = whites * spp if linear and len(whites) == 1 else whites
    if linear and not all(1 <= v <= maxv for v in whites):
        raise InvalidOptionError("WhiteLevel", tuple(whites), f"it lies outside [1, {maxv}]")
    white = max(whites) if linear else whites[0]      # (a mosaic reads the first value; the shift follows the largest)
    if not 1 <= white <= maxv:
        raise InvalidOptionError("WhiteLevel", white, f"it lies outside [1, {maxv}]")
    shift = max(0, 8 * dt.itemsize - white.bit_length())
    layout.shift = shift
    if 50712 in rawifd:
        if bits == 8:
            raise InvalidOptionError("LinearizationTable", "present", "a table on 8-bit samples is not read (its entries are 16-bit)")
        table = np.array(t.take(rawifd, 50712, 1, integral=True), np.int64)
        if not 1 <= len(table) <= MAX_TABLE or table.min() < 0 or table.max() > 65535:
            raise InvalidOptionError("LinearizationTable", len(table), f"1 to {MAX_TABLE} entries of 16 bits are expected")
        layout.table = table.astype(np.uint16)
    brep = tuple(get(50713, (1, 1), integral=True))
    if linear and brep != (1, 1):
        raise InvalidOptionError("BlackLevelRepeatDim", brep, "only 1 x 1 is read for a LinearRaw frame")
    if brep not in ((1, 1), (2, 2)):
        raise InvalidOptionError("BlackLevelRepeatDim", brep, "1 x 1 or 2 x 2 is read")
    neutral = get(50728)

    def check_neutral():
        if neutral is not None and (len(neutral) != 3 or min(neutral) <= 0):
            raise InvalidOptionError("AsShotNeutral", tuple(neutral), "three positive values are expected")
    cfa = lin = black = None
    if linear:
        check_neutral()
        bl = [int(np.floor(float(v) + 0.5)) for v in get(50714, (0,))]
        if len(bl) not in (1, spp):
            raise InvalidOptionError("BlackLevel", bl, f"one value, or one per sample ({spp}), is expected")
        bl = bl * spp if len(bl) == 1 else bl
        if min(bl) < 0 or any(b >= w for b, w in zip(bl, whites)):
            raise InvalidOptionError("BlackLevel", bl, f"it lies outside [0, WhiteLevel = {tuple(whites)})")
        gains = []
        for c in range(spp):
            wb = 1.0 if neutral is None or spp == 1 else float(neutral[1]) / float(neutral[c])
            gains.append(wb * maxv / float((whites[c] - bl[c]) << shift))
        lin = Linear(black=[b << shift for b in bl], gains=gains, white=None, spp=spp)
    else:
        bl = [int(np.floor(float(v) + 0.5)) for v in get(50714, (0,) * (brep[0] * brep[1]))]
        if len(bl) != brep[0] * brep[1]:
            raise InvalidOptionError("BlackLevel", bl, f"{brep[0] * brep[1]} values are expected")
        black = bl * 4 if len(bl) == 1 else bl       # (its origin is the ActiveArea's: already in the crop's coordinates)
        if min(black) < 0 or max(black) >= white:
            raise InvalidOptionError("BlackLevel", black, f"it lies outside [0, WhiteLevel = {white})")

        # colour
        pattern = permute_pattern(pattern, layout.crop_y, layout.crop_x)
        check_neutral()
        gains = []
        for pos in range(4):
            wb = 1.0 if neutral is None else float(neutral[1]) / float(neutral["RGB".index(pattern[pos])])
            gains.append(wb * maxv / float((white - black[pos]) << shift))
        cfa = Cfa(pattern, black=[b << shift for b in black], gains=gains, white=None)
    mats = {k: get(tag) for k, tag in ((1, 50721), (2, 50722))}
    ill = {1: _one(t, ifd0, 50778, _one(t, rawifd, 50778, None)), 2: _one(t, ifd0, 50779, _one(t, rawifd, 50779, None))}
    pick = next((k for k in (1, 2) if mats[k] is not None and ill[k] == D65), None)
    if pick is None:
        pick = 2 if mats[2] is not None else 1 if mats[1] is not None else None
    develop = None
    if pick is not None:
        if len(mats[pick]) != 9:
            raise InvalidOptionError(f"ColorMatrix{pick}", len(mats[pick]), "a 3 x 3 matrix is expected")
        develop = Develop(matrix=colour_matrix(mats[pick]), tone=srgb_tone(dt))

    # what is in the file and not applied
    ignored = [TAG_NAMES[tag] for tag in IGNORED_TAGS if tag in rawifd or tag in ifd0]
    lens, ops2, ops3 = None, [], []
    for tag in (51008, 51009, 51022):
        if tag not in rawifd and tag not in ifd0:
            continue
        name = TAG_NAMES[tag]
        ops = _opcodes(t.raw((rawifd if tag in rawifd else ifd0)[tag]), name, path)
        if tag == 51009:
            ops2 = ops
        if tag == 51022:
            ops3 = ops
        if tag != 51022:
            ignored.append(name)
        for oid, body in ops:
            oname = OPCODE_NAMES.get(oid, f"Opcode{oid}")
            if tag == 51022 and oid == 1 and lens is None:
                lens = _warp_rectilinear(body, layout.height, layout.width // spp, path)
                if lens is not None:
                    continue
                oname = "WarpRectilinear (tangential terms)"
            ignored.append(oname)
    orientation = int(_one(t, ifd0, 274, _one(t, rawifd, 274, 1)))
    if not 1 <= orientation <= 8:
        raise InvalidOptionError("Orientation", orientation, "valid values are 1 to 8")
    corrections = _site_corrections(t, rawifd, ifd0, ops2, layout, black, path)
    finish = _file_finish(t, rawifd, ifd0, ops3, (layout.height, layout.width // spp), lens, orientation, linear=linear)
    return DngFrame(path, layout, span, cfa, develop, lens, orientation, ignored, corrections, finish, linear=lin)


def _warp_rectilinear(body, h, w, path):
    """the opcode's data -- uint32 planes, six doubles per plane (kr0..kr3, kt0, kt1), the centre as two doubles in [0, 1] of
    the image -- as a lens.Lens; None when a tangential term is not 0 (not modelled)"""
    from .lens import Lens
    if len(body) < 4:
        raise ImageLoadError(path, "WarpRectilinear is shorter than its plane count")
    n = struct.unpack(">I", body[:4])[0]
    if n not in (1, 3) or len(body) < 4 + 8 * (6 * n + 2):
        raise ImageLoadError(path, f"WarpRectilinear with {n} planes in {len(body)} bytes")
    vals = struct.unpack(f">{6 * n + 2}d", body[4:4 + 8 * (6 * n + 2)])
    planes = [vals[6 * i:6 * i + 6] for i in range(n)]
    if any(p[4] != 0.0 or p[5] != 0.0 for p in planes):
        return None
    cx, cy = vals[6 * n], vals[6 * n + 1]
    return Lens.from_warp_rectilinear(planes[0] if n == 1 else planes, centre=(cx * (w - 1), cy * (h - 1)))


# ---------------------------------------------------------------- lossless JPEG: the headers of one segment
SOF_NAMES = {0xC0: "SOF0 baseline DCT", 0xC1: "SOF1 extended sequential DCT", 0xC2: "SOF2 progressive DCT", 0xC5: "SOF5 differential DCT",
             0xC6: "SOF6 differential progressive DCT", 0xC7: "SOF7 differential lossless", 0xC9: "SOF9 arithmetic DCT",
             0xCA: "SOF10 arithmetic progressive DCT", 0xCB: "SOF11 arithmetic lossless", 0xCD: "SOF13 differential arithmetic DCT",
             0xCE: "SOF14 differential arithmetic progressive DCT", 0xCF: "SOF15 differential arithmetic lossless"}
LJPEG_HEADER_MAX = 65536           # (markers are looked for this far into a segment: headers are a few hundred bytes)


def _ljpeg_segment(rec, k, span, off, count, bits, rows, seg_w, nfs=(1, 2)):
    """Fill the descriptor `rec` (a one-element LJPEG_SEG_DTYPE view) of segment k, the `count` bytes of `span` from `off`,
    from the stream's markers: SOI, DHT / DRI / anything with a length, SOF3, SOS.  Only the markers are read out of the
    mapping, four bytes and then the marker's own length at a time: the sample data is not touched.  The entropy-coded data
    is everything behind the SOS header up to the segment's end: the decoder stops at the first marker inside it."""
    def refuse(what):
        raise InvalidOptionError("Compression", 7, f"lossless JPEG: segment {k}: {what}")

    def take(a, n):     # n bytes from byte a of the segment, fewer at its end
        return bytes(span[off + a:off + min(a + n, count)])
    if take(0, 2) != b"\xff\xd8":
        refuse("it does not start with SOI (FF D8): found " + (take(0, 2).hex(" ").upper() or "nothing"))
    at, dht, frame = 2, {}, None
    while True:
        h4 = take(at, 4)
        if len(h4) < 4 or at > LJPEG_HEADER_MAX:
            refuse(f"the headers end at byte {at} without a scan (SOS)")
        if h4[0] != 0xFF:
            refuse(f"byte {h4[0]:#04x} at {at} where a marker is expected")
        m = h4[1]
        if m == 0xFF:           # fill
            at += 1
            continue
        n = h4[2] << 8 | h4[3]
        body = take(at + 4, n - 2) if n >= 2 else b""
        if n < 2 or len(body) != n - 2:
            refuse(f"marker FF {m:02X} at {at} with length {n} runs past the segment")
        if m == 0xC4:
            i = 0
            while i < len(body):
                counts = list(body[i + 1:i + 17])
                values = list(body[i + 17:i + 17 + sum(counts)])
                if len(counts) != 16 or len(values) != sum(counts):
                    refuse(f"a DHT at {at} is cut short")
                code = 0
                for length, c in enumerate(counts, 1):
                    code += c
                    if code > 1 << length:
                        refuse(f"the DHT of table {body[i] & 15} overflows the code space at length {length}")
                    code <<= 1
                if not 1 <= len(values) <= 17:
                    refuse(f"the DHT of table {body[i] & 15} holds {len(values)} values (1 to 17 are expected)")
                if max(values) > 16:
                    refuse(f"the DHT of table {body[i] & 15} holds the category {max(values)} (at most 16)")
                if body[i] >> 4 == 0:
                    dht[body[i] & 15] = (counts, values)
                i += 17 + len(values)
        elif m == 0xC3:
            if len(body) < 6 or len(body) < 6 + 3 * body[5]:
                refuse("SOF3 is cut short")
            frame = (body[0], body[1] << 8 | body[2], body[3] << 8 | body[4], body[5], [body[6 + 3 * i] for i in range(body[5])])
        elif m in SOF_NAMES:
            refuse(f"the frame is {SOF_NAMES[m]}, not SOF3 lossless")
        elif m == 0xDD:
            if len(body) >= 2 and (body[0] << 8 | body[1]) != 0:
                refuse(f"DRI with a restart interval of {body[0] << 8 | body[1]} (restart intervals are not read)")
        elif m == 0xDA:
            break
        at += 2 + n
    if frame is None:
        refuse("SOS without a frame (SOF3) in front of it")
    prec, lines, x, nf, ids = frame
    if nf not in nfs:
        refuse(f"Nf = {nf} components (1 or 2 are read)" if nfs == (1, 2) else
               f"Nf = {nf} components (a LinearRaw frame of 3 samples per pixel is read from streams of Nf = 3)")
    if x * nf != seg_w or lines != rows:
        refuse(f"a frame of {lines} lines of {x} x {nf} samples does not match its segment of {rows} x {seg_w}")
    if not 2 <= prec <= bits:
        refuse(f"P = {prec} with BitsPerSample = {bits} (2 <= P <= BitsPerSample)")
    if len(body) < 1 or body[0] != nf or len(body) < 4 + 2 * nf:
        refuse(f"a scan of Ns = {body[0] if body else None} components for Nf = {nf} (one scan with Ns == Nf is read)")
    sel = {body[1 + 2 * i]: body[2 + 2 * i] >> 4 for i in range(nf)}
    pred, al = body[1 + 2 * nf], body[3 + 2 * nf] & 15
    if al != 0:
        refuse(f"Al = {al} (point transforms are not read)")
    if not 1 <= pred <= 7:
        refuse(f"predictor Ss = {pred} (1 to 7)")
    if pred != 1 and seg_w > _lib.LJPEG_MAX_LINE:
        refuse(f"predictor Ss = {pred} on a segment of {seg_w} columns (predictors 2 to 7 are read up to {_lib.LJPEG_MAX_LINE})")
    r = rec[0]
    for c, cid in enumerate(ids):
        if cid not in sel or sel[cid] not in dht:
            refuse(f"component {cid} selects table {sel.get(cid)}, which no DHT defines")
        counts, values = dht[sel[cid]]
        r["counts"][c, :] = counts
        r["values"][c, :len(values)] = values
    scan = at + 2 + n
    r["scan_off"], r["scan_bytes"] = off + scan, count - scan
    r["x"], r["y"], r["ncomp"], r["predictor"], r["precision"] = x, lines, nf, pred, prec


# ---------------------------------------------------------------- the device side
def host_span(frame):
    """the frame's span as memory a plain (pageable) upload may read: a read-only file mapping is copied once on the host --
    the runtime pins what it uploads, and read-only pages do not pin.  (Stack.push_packed on an asynchronous handle needs no
    such copy: there the library copies the mapping into its own pinned bounce buffer.)"""
    return frame.span if frame.span.flags.writeable else np.array(frame.span)


def _check_frame(frame):
    if not isinstance(frame, DngFrame):
        raise InvalidOptionError("frame", frame, "a shinestacker_amd.dng.DngFrame (dng.read) is expected")
    return frame


def check_linear_options(frame, calibration=None, corrections=None, develop=None, finish=None):
    """What a LinearRaw `frame` does not take, refused by name: a Calibration, Develop.defects, a SiteCorrections object that
    holds anything and a Finish with a vignette are all per CFA site.  ("auto" is fine: the file's own per-site corrections
    are then recorded as skipped, `corrections.skipped` / `finish.skipped`, with the reason "LinearRaw frame".)"""
    if calibration is not None:
        raise InvalidOptionError("calibration", calibration, f"{frame.path}: calibration frames are per CFA site: a LinearRaw frame has none")
    if corrections is not None and not isinstance(corrections, str) and not check_corrections(corrections).empty:
        raise InvalidOptionError("corrections", corrections, f"{frame.path}: site corrections are per CFA site: a LinearRaw frame has none")
    if develop is not None and not isinstance(develop, str) and develop.defects is not None:
        raise InvalidOptionError("develop", develop, f"{frame.path}: Develop.defects lists the sites of a CFA mosaic: a LinearRaw frame has none")
    fin = resolve_finish(frame, finish)
    if fin is not None and fin.vignette is not None:
        raise InvalidOptionError("finish", fin, f"{frame.path}: Finish.vignette is a gain on the sites of a CFA mosaic: a LinearRaw frame has none")
    return fin


def unpack(frame, device=0, corrections=None, finish=None, split=False):
    """The cropped H x W mosaic of a DngFrame as a NumPy array of its dtype: span up, raw_unpack or raw_ljpeg, mosaic down.
    `split`: False, True or {"sub_bytes": ..., "max_rounds": ...} -- a lossless-JPEG frame of one or two components is decoded
    by the split path (csrc/kernels_ljpeg_split.hpp: the same samples); anything else ignores it.
    A lossless-JPEG frame one of whose streams did not decode raises ImageLoadError.  `corrections`: None, "auto" (the
    frame's own) or a SiteCorrections, applied to the unpacked mosaic (demosaic.correct_sites).  `finish`: None, "auto" or
    a Finish -- its VIGNETTE only, behind the corrections (demosaic.radial_gain; no lens follows here: the table is the
    polynomial itself); crop and orientation belong to the developed frame (`develop`).
    A LinearRaw frame: its H x W x 3 samples in file order (R, G, B), or H x W at one sample per pixel -- the layout counts
    samples, so the same kernel decodes them; a SiteCorrections object or a vignette is refused (check_linear_options)."""
    if _check_frame(frame).linear is not None:
        check_linear_options(frame, corrections=corrections, finish=finish)
        h, w = frame.shape
        return _unpack_plane(frame, device, split).reshape((h, w, 3) if frame.layout.spp == 3 else (h, w))
    fin = resolve_finish(_check_frame(frame), finish)
    if fin is not None and fin.vignette is not None:
        from .demosaic import radial_gain
        return radial_gain(unpack(frame, device, corrections, split=split), frame.cfa, fin.vignette, device=device)
    sc = resolve_corrections(_check_frame(frame), corrections)
    if sc is not None:
        from .demosaic import correct_sites
        return correct_sites(unpack(frame, device, split=split), frame.cfa, sc, device=device)
    return _unpack_plane(frame, device, split)


def takes_split(layout, split):
    """whether `split` sends this layout through the split path: lossless JPEG of one or two components"""
    return bool(split) and layout.compression == 7 and layout.spp != 3


def split_options(layout, span_bytes, split):
    """(the JpegSplitStruct a device form is called with, the scratch bytes it needs) for a layout whose descriptors lie in
    host memory too: max_rounds 0 becomes the exact bound -- the largest number of workgroups of 256 subsequences any one
    segment's lanes touch, minus 1 -- so that the device form never leaves a segment unsynced"""
    opt = _lib.ljpeg_split_options(split)
    opt = _lib.JpegSplitStruct(opt.sub_bytes, opt.max_rounds)
    if opt.max_rounds == 0:
        sub = opt.sub_bytes or 128
        off = layout.segments["scan_off"].astype(np.int64)
        length = np.clip(np.minimum(layout.segments["scan_bytes"].astype(np.int64), int(span_bytes) - off), 0, None)
        lanes = np.maximum(1, -(-length // sub))
        last = np.cumsum(lanes) - 1
        first = last - lanes + 1
        opt.max_rounds = int((last // 256 - first // 256).max())      # (0 asks for the default: rounds not needed return at once)
    nbytes = _lib.C.c_size_t(0)
    L = layout.struct()
    _lib.check(_lib.load().mi_ljpeg_split_scratch_bytes(_lib.C.byref(L), int(span_bytes), _lib.C.byref(opt), _lib.C.byref(nbytes)))
    return opt, int(nbytes.value)


def _unpack_plane(frame, device, split=False):
    """layout.height x layout.width samples of the frame's span (a mosaic; of a LinearRaw frame the H x (W spp) samples)"""
    lay = _check_frame(frame).layout
    _lib.require_device()
    out = np.empty((lay.height, lay.width), lay.dtype)
    L = lay.struct()
    span = host_span(frame)
    if lay.compression == 7:
        status = np.zeros(len(lay.segments), np.uint32)
        if takes_split(lay, split):
            opt = _lib.ljpeg_split_options(split)
            _lib.check(_lib.load().mi_raw_ljpeg_split(device, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, _lib.C.byref(L),
                                                      None if lay.table is None else lay.table.ctypes.data, _lib.C.byref(opt),
                                                      out.ctypes.data, status.ctypes.data))
            check_ljpeg_status(frame.path, status)
            return out
        entry = _lib.load().mi_raw_ljpeg3 if lay.spp == 3 else _lib.load().mi_raw_ljpeg
        _lib.check(entry(device, span.ctypes.data, span.nbytes, lay.segments.ctypes.data, _lib.C.byref(L),
                                            None if lay.table is None else lay.table.ctypes.data, out.ctypes.data, status.ctypes.data))
        check_ljpeg_status(frame.path, status)
        return out
    _lib.check(_lib.load().mi_raw_unpack(device, span.ctypes.data, span.nbytes, lay.offsets.ctypes.data, _lib.C.byref(L),
                                         None if lay.table is None else lay.table.ctypes.data, out.ctypes.data))
    return out


def check_ljpeg_status(path, status):
    """ImageLoadError naming the first flagged segment of `status` (one word per segment, or one word for a whole stack)"""
    status = np.atleast_1d(np.asarray(status))
    bad = np.flatnonzero(status)
    if len(bad):
        k = int(bad[0])
        where = f"segment {k}" if len(status) > 1 or k else "a segment"
        raise ImageLoadError(path, f"lossless JPEG: {where} did not decode (status {int(status[k])}: {_lib.ljpeg_flag_text(int(status[k]))})")


def unpack_device(layout, dev_span, span_bytes, dev_offsets, dev_table, dev_out, device=0, stream=None, dev_status=None, split=False,
                  dev_scratch=None):
    """raw_unpack on buffers resident in HBM: the span (`span_bytes` of it, 4-byte aligned), the uint32 segment offsets, the
    uint16 table (or None) -> `dev_out`, layout.height x layout.width samples.  Queued on `stream`, not waited for.  A
    lossless-JPEG layout: `dev_offsets` holds its descriptors (layout.segments, 16-byte aligned) and raw_ljpeg runs, which
    leaves one status word per segment at `dev_status` (or None).  `split` (False, True or a dict, as `unpack` takes it) sends
    a lossless-JPEG layout of one or two components through the split path: `dev_scratch` is then a _lib.DeviceBuffer of at
    least split_options(layout, span_bytes, split)[1] bytes, which the queued kernels use until they are through."""
    _lib.require_device()
    L = layout.struct()
    if takes_split(layout, split):
        opt, need = split_options(layout, span_bytes, split)
        if dev_scratch is None or dev_scratch.nbytes < need:
            raise InvalidOptionError("dev_scratch", dev_scratch, f"the split path needs a DeviceBuffer of at least {need} bytes")
        _lib.check(_lib.load().mi_raw_ljpeg_split_device(device, stream, dev_span, int(span_bytes), dev_offsets, _lib.C.byref(L), dev_table,
                                                         _lib.C.byref(opt), dev_scratch.ptr, dev_scratch.nbytes, dev_out, dev_status))
        return
    if layout.compression == 7:     # (three samples per pixel: mi_ljpeg_seg3_t descriptors and raw_ljpeg3)
        entry = _lib.load().mi_raw_ljpeg3_device if layout.spp == 3 else _lib.load().mi_raw_ljpeg_device
        _lib.check(entry(device, stream, dev_span, int(span_bytes), dev_offsets, _lib.C.byref(L), dev_table, dev_out, dev_status))
        return
    _lib.check(_lib.load().mi_raw_unpack_device(device, stream, dev_span, int(span_bytes), dev_offsets, _lib.C.byref(L), dev_table, dev_out))


class _Staged:
    """a frame's span, offsets (or lossless-JPEG descriptors and status words) and table in one device buffer; with `split`
    (as `unpack` takes it) the split path's scratch too, in a buffer of its own (`free` releases both)"""

    def __init__(self, frame, device, split=False):
        lay = frame.layout
        self.split = split if takes_split(lay, split) else False
        self.scratch = None
        segs = lay.segments if lay.compression == 7 else lay.offsets
        self.path, self.nseg = frame.path, len(segs)
        self.seg_at = (frame.span.nbytes + 255) & ~255
        self.status_at = self.seg_at + ((segs.nbytes + 255) & ~255)
        self.table_at = self.status_at + (((4 * self.nseg + 255) & ~255) if lay.compression == 7 else 0)
        self.buf = _lib.DeviceBuffer(self.table_at + (0 if lay.table is None else lay.table.nbytes), device)
        self.buf.upload(host_span(frame))
        self.buf.upload(segs, self.seg_at)
        self.status = self.buf.ptr + self.status_at if lay.compression == 7 else None
        if lay.table is not None:
            self.buf.upload(lay.table, self.table_at)
        self.span_bytes = frame.span.nbytes
        self.table = None if lay.table is None else self.buf.ptr + self.table_at
        if self.split:
            try:
                self.scratch = _lib.DeviceBuffer(split_options(lay, self.span_bytes, self.split)[1], device)
            except Exception:
                self.buf.free()
                raise
            span_free = self.buf.free

            def free():         # (callers release `buf`: the scratch goes with it)
                span_free()
                self.scratch.free()
            self.buf.free = free

    def unpack_into(self, layout, dev_out, device, stream=None):
        if self.split:
            unpack_device(layout, self.buf.ptr, self.span_bytes, self.buf.ptr + self.seg_at, self.table, dev_out, device, stream, self.status,
                          split=self.split, dev_scratch=self.scratch)
            return
        unpack_device(layout, self.buf.ptr, self.span_bytes, self.buf.ptr + self.seg_at, self.table, dev_out, device, stream, self.status)

    def check_status(self):
        """after a wait for the kernel: ImageLoadError when a lossless-JPEG segment did not decode"""
        if self.status is not None:
            check_ljpeg_status(self.path, self.buf.download((self.nseg,), np.uint32, self.status_at))


def _resolve(frame, develop, lens):
    from .demosaic import check_develop
    from .lens import check_lens
    if isinstance(develop, str):
        if develop != "auto":
            raise InvalidOptionError("develop", develop, '"auto", None or a demosaic.Develop is expected')
        develop = frame.develop
    elif develop is not None:
        check_develop(develop)
    if isinstance(lens, str):
        if lens != "auto":
            raise InvalidOptionError("lens", lens, '"auto", None or a lens.Lens is expected')
        lens = frame.lens
    elif lens is not None:
        lens = check_lens(lens)
    return develop, lens


def develop(frame, develop="auto", lens="auto", calibration=None, device=0, corrections=None, finish=None, split=False):
    """A DngFrame -> H x W x 3 BGR of its dtype: unpack, then `debayer` with the frame's own Cfa.  `develop`, `lens`: "auto"
    takes frame.develop / frame.lens, None switches the step off, an object overrides it.  `calibration`: a
    demosaic.Calibration applied to the unpacked mosaic first.  `corrections`: None, "auto" or a SiteCorrections -- the
    file's site corrections, ahead of the calibration.  `finish`: None, "auto" or a Finish -- the vignette gain behind the
    corrections, crop and orientation last: the result is then H' x W' x 3 (`DngFrame.finished_shape`).  `split`: as `unpack`
    takes it."""
    if split:
        mosaic = unpack(_check_frame(frame), device, split=split)
        return _develop_unpacked(frame, mosaic, develop, lens, calibration, device, corrections, finish)
    dev, ln = _resolve(_check_frame(frame), develop, lens)
    if frame.linear is not None:    # no mosaic: the samples straight into linear_develop; crop and orientation apply
        fin = check_linear_options(frame, calibration, corrections, dev, finish)
        return develop_linear(unpack(frame, device), frame.linear, develop=dev, lens=ln, finish=fin, device=device)
    sc = resolve_corrections(frame, corrections)
    fin = resolve_finish(frame, finish)
    if fin is not None:
        try:
            return debayer(unpack(frame, device), frame.cfa, develop=dev, device=device, calibration=calibration, lens=ln, corrections=sc,
                           finish=fin)
        finally:
            if fin is frame.finish:
                fin.close()     # (the file's own table: debayer has waited for the device)
    if sc is not None:
        return debayer(unpack(frame, device), frame.cfa, develop=dev, device=device, calibration=calibration, lens=ln, corrections=sc)
    return debayer(unpack(frame, device), frame.cfa, develop=dev, device=device, calibration=calibration, lens=ln)


def _develop_unpacked(frame, mosaic, develop, lens, calibration, device, corrections, finish):
    """`develop` behind the unpack: `mosaic` is what unpack(frame, device) returns, decoded by whichever path"""
    dev, ln = _resolve(frame, develop, lens)
    if frame.linear is not None:
        fin = check_linear_options(frame, calibration, corrections, dev, finish)
        return develop_linear(mosaic, frame.linear, develop=dev, lens=ln, finish=fin, device=device)
    sc = resolve_corrections(frame, corrections)
    fin = resolve_finish(frame, finish)
    if fin is not None:
        try:
            return debayer(mosaic, frame.cfa, develop=dev, device=device, calibration=calibration, lens=ln, corrections=sc, finish=fin)
        finally:
            if fin is frame.finish:
                fin.close()
    if sc is not None:
        return debayer(mosaic, frame.cfa, develop=dev, device=device, calibration=calibration, lens=ln, corrections=sc)
    return debayer(mosaic, frame.cfa, develop=dev, device=device, calibration=calibration, lens=ln)


def frames_device(paths, dev_out, develop="auto", lens="auto", calibration=None, device=0, corrections=None, finish=None, split=False):
    """Read the n DNG files (equal cropped shape and dtype), upload their spans and unpack and demosaic them side by side
    into `dev_out` (device pointer, n x H x W x 3 of their dtype): exactly what pipeline.align_and_stack_device(dev_frames,
    ...) takes, as demosaic.debayer_frames_device does for mosaics.  Waits for the device.  Returns (H, W, dtype).
    `corrections`: None, "auto" (each file's own) or a SiteCorrections, applied in place behind the unpack.
    `finish`: None, "auto" (each file's own) or a Finish: the frames in `dev_out` are then n x H' x W' x 3, the finished
    shape, which every file must share, and (H', W', dtype) is returned.  `split`: as `unpack` takes it."""
    if len(paths) == 0:
        raise ValueError("no files")
    _lib.require_device()
    first = None
    stage = scratch = fscratch = None
    out_shape = None
    try:
        for i, p in enumerate(paths):
            frame = read(p)
            if first is None:
                first = frame
                h, w = frame.shape
                frame_bytes = h * w * 3 * frame.dtype.itemsize
            elif frame.shape != first.shape or frame.dtype != first.dtype:
                raise InvalidOptionError("paths", p, f"a {frame.shape} {frame.dtype} frame among {first.shape} {first.dtype} ones")
            stage_bytes = h * w * frame.layout.spp * frame.dtype.itemsize      # (a LinearRaw frame: spp samples per pixel)
            if stage is None or stage.nbytes < stage_bytes:
                if stage is not None:
                    stage.free()        # (the device was waited for behind the frame before)
                stage = _lib.DeviceBuffer(stage_bytes, device)
            dev, ln = _resolve(frame, develop, lens)
            if frame.linear is not None:
                check_linear_options(frame, calibration, corrections, dev, finish)
            if ln is not None and scratch is None:
                scratch = _lib.DeviceBuffer(frame_bytes, device)
            fin = resolve_finish(frame, finish)
            if finish is not None:
                shape = frame.shape if fin is None else fin.finished_shape(frame.shape)
                if out_shape is None:
                    out_shape = shape
                elif shape != out_shape:
                    raise InvalidOptionError("paths", p, f"a frame finished to {shape} among ones finished to {out_shape}")
                out_bytes = out_shape[0] * out_shape[1] * 3 * frame.dtype.itemsize
                if fin is not None and fscratch is None:
                    fscratch = _lib.DeviceBuffer(frame_bytes, device)
            up = _Staged(frame, device, split) if split else _Staged(frame, device)
            try:
                up.unpack_into(frame.layout, stage.ptr, device)
                sc = None if frame.linear is not None else resolve_corrections(frame, corrections)
                if sc is not None:
                    from .demosaic import correct_sites_device
                    correct_sites_device(stage.ptr, h, w, frame.dtype, frame.cfa, sc, device=device)
                if frame.linear is not None:
                    develop_linear_device(stage.ptr, dev_out + i * (frame_bytes if fin is None else out_bytes), h, w, frame.dtype,
                                          frame.linear, device=device, develop=dev, lens=ln, lens_scratch=scratch, finish=fin,
                                          finish_scratch=fscratch)
                elif fin is not None:
                    debayer_device(stage.ptr, dev_out + i * out_bytes, h, w, frame.dtype, frame.cfa, device=device, develop=dev,
                                   calibration=calibration, lens=ln, lens_scratch=scratch, finish=fin, finish_scratch=fscratch)
                else:
                    debayer_device(stage.ptr, dev_out + i * frame_bytes, h, w, frame.dtype, frame.cfa, device=device, develop=dev,
                                   calibration=calibration, lens=ln, lens_scratch=scratch)
                # the stage and the staged span are reused / freed: the null stream's kernels must be through first
                _lib.check(_lib.load().mi_device_synchronize(device))
                up.check_status()
            finally:
                up.buf.free()
                if isinstance(corrections, str) and frame.corrections is not None:
                    frame.corrections.close()     # (the device was waited for above, or nothing was queued)
                if isinstance(finish, str):
                    frame.finish.close()
    finally:
        for buf in (stage, scratch, fscratch):
            if buf is not None:
                buf.free()
    if out_shape is not None:
        return out_shape[0], out_shape[1], first.dtype
    return h, w, first.dtype
