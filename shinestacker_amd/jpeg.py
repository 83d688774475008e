"""Baseline JPEG frames decoded on the device (csrc/kernels_jpeg.hpp; no reference counterpart: the reference decodes on the
host through OpenCV).

`read(path)` maps the file and reads its headers -- struct and NumPy only, no codec -- into a JpegFrame: the entropy-coded
scan as it lies in the file (`span`), where its restart intervals start (`offsets`), and the mi_jpeg_t the kernels take
(`desc`).  The span goes up to the device as it is, a fifth of the decoded frame at quality 95; the kernels decode the Huffman symbols of
every restart interval independently, run the inverse DCT, upsample the chroma and convert to the H x W x 3 BGR uint8 frame
`imageio.read_img` returns for the same file (bit for bit where libjpeg-turbo is the host decoder).

What is decoded: SOF0 (and SOF1 with 8-bit precision, Huffman coded), one interleaved scan of 1 or 3 components, luma
sampling (1,1), (2,1) or (2,2) with chroma (1,1), 8-bit quantisation tables, DC and AC tables 0 and 1, a restart interval,
and a colour space libjpeg's rule reads as YCbCr or grey (JFIF: YCbCr; else an Adobe segment with transform 1; else component
ids 1, 2, 3).  Everything else is refused by `read` with InvalidOptionError, naming the marker and the value found, before
any device call -- among it, by default, files WITHOUT a restart interval, whose single interval would be one serial walk, and
files whose interval is longer than MAX_DRI MCUs (the MCU row of a picture 65 535 wide), for the same reason.

`read(path, split="needed")` takes those two kinds of file as well and marks them (`JpegFrame.split`) for the split decoder
(csrc/kernels_jpeg_split.hpp), which cuts an interval of any length into subsequences, decodes them on many lanes at once and
repairs the lanes' guesses until the result is exact; `split="always"` sends every file there.  Still refused either way:
progressive and arithmetic-coded files, 12-bit samples, CMYK and RGB components, several scans, fill bytes inside the scan.

EXIF orientation is reported (`JpegFrame.orientation`) and not applied, as the Pillow branch of read_img leaves it.
"""
import mmap
import struct

import numpy as np

from . import _lib
from .errors import ImageLoadError, InvalidOptionError

EXTENSIONS = ("jpg", "jpeg")
MODES = (None, "device", "auto")
SPLIT = (None, "needed", "always")
MAX_DRI = 8192      # MI_JPEG_MAX_DRI: MCUs in the longest interval that is decoded
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
           49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_SOF = {0xC2: "SOF2 (progressive DCT)", 0xC3: "SOF3 (lossless)", 0xC5: "SOF5 (differential DCT)", 0xC6: "SOF6 (differential progressive)",
        0xC7: "SOF7 (differential lossless)", 0xC9: "SOF9 (arithmetic coding)", 0xCA: "SOF10 (arithmetic coding, progressive)",
        0xCB: "SOF11 (arithmetic coding, lossless)", 0xCD: "SOF13 (arithmetic coding, differential)",
        0xCE: "SOF14 (arithmetic coding, differential progressive)", 0xCF: "SOF15 (arithmetic coding, differential lossless)"}


def is_jpeg(path):
    return str(path).split(".")[-1] in EXTENSIONS


def check_mode(mode):
    if mode not in MODES:
        raise InvalidOptionError("jpeg", mode, 'None, "device" or "auto" is expected')
    return mode


class JpegFrame:
    """What `read` found.  shape (H, W), dtype uint8, ncomp 1 or 3, sampling (hmax, vmax), dri (MCUs per restart interval),
    span (the scan's bytes, a view of the file's mapping), offsets (uint32, n_intervals + 1, into the span), desc (the
    _lib.JpegStruct the kernels take), orientation (the EXIF tag, 1 when absent; not applied).  split: whether the frame goes to
    the split decoder (read's `split=`); then dri is 0 for a file without a restart interval, desc.dri the MCU count and there
    is one interval.  split_options: (sub_bytes, max_rounds) for that decoder, 0 for the library's default."""

    def __init__(self, path, shape, ncomp, sampling, dri, span, offsets, desc, orientation, keep, split=False):
        self.split, self.split_options = split, (0, 0)
        self.path, self.shape, self.dtype = path, shape, np.dtype(np.uint8)
        self.ncomp, self.sampling, self.dri = ncomp, sampling, dri
        self.span, self.offsets, self.desc, self.orientation = span, offsets, desc, orientation
        self.n_intervals = len(offsets) - 1
        self._keep = keep

    def coef_shapes(self):
        """per component (rows of blocks, blocks a row, 64): its padded coefficient plane"""
        (h, w), (hm, vm) = self.shape, self.sampling
        mx, my = -(-w // (8 * hm)), -(-h // (8 * vm))
        return [(my * (vm if c == 0 else 1), mx * (hm if c == 0 else 1), 64) for c in range(self.ncomp)]


def _refuse(path, marker, value, why):
    return InvalidOptionError(marker, value, f"{path}: {why}")


def _exif_orientation(tiff):
    try:
        e = "<" if tiff[:2] == b"II" else ">"
        off = struct.unpack(e + "I", tiff[4:8])[0]
        for i in range(struct.unpack(e + "H", tiff[off:off + 2])[0]):
            tag, typ, _ = struct.unpack(e + "HHI", tiff[off + 2 + 12 * i:off + 10 + 12 * i])
            if tag == 0x0112 and typ == 3:
                v = struct.unpack(e + "H", tiff[off + 10 + 12 * i:off + 12 + 12 * i])[0]
                return v if 1 <= v <= 8 else 1
    except struct.error:
        pass
    return 1


def read(path, split=None):
    """The headers of a baseline JPEG file -> JpegFrame; InvalidOptionError for everything the device decoder does not take
    (the module docstring lists it), RuntimeError when the file does not exist, as read_img.  split: None -- a file without a
    restart interval, or with one longer than MAX_DRI, is refused; "needed" -- such a file is taken and marked for the split
    decoder; "always" -- every file is."""
    import os
    if split not in SPLIT:
        raise InvalidOptionError("split", split, 'None, "needed" or "always" is expected')
    path = str(path)
    if not os.path.isfile(path):
        raise RuntimeError("File does not exist: " + path)
    with open(path, "rb") as fh:
        size = os.fstat(fh.fileno()).st_size
        if size < 4:
            raise _refuse(path, "SOI", size, "a file of that many bytes holds no image")
        mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
    data = np.frombuffer(mm, np.uint8)
    if bytes(data[:2]) != b"\xff\xd8":
        raise _refuse(path, "SOI", bytes(data[:2]).hex(), "the file does not start with FF D8")
    quant, tables = {}, {}
    dri, jfif, adobe, orientation, sof, scan = 0, False, None, 1, None, None
    pos = 2
    while scan is None:
        if pos + 2 > size:
            raise _refuse(path, "SOS", "none", "the file ends before a scan starts")
        if data[pos] != 0xFF:
            raise _refuse(path, "marker", f"{int(data[pos]):02x} at byte {pos}", "FF is expected where a segment ends")
        m = int(data[pos + 1])
        if m == 0xFF:
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:      # (no length behind these)
            pos += 2
            continue
        if m == 0xD9:
            raise _refuse(path, "EOI", f"byte {pos}", "the image ends before a scan starts")
        if pos + 4 > size:
            raise _refuse(path, "SOS", "none", "the file ends before a scan starts")
        n = (int(data[pos + 2]) << 8) | int(data[pos + 3])
        if n < 2 or pos + 2 + n > size:
            raise _refuse(path, f"marker FF{m:02X}", n, "its length runs past the end of the file")
        body = bytes(data[pos + 4:pos + 2 + n])
        if m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq != 0:
                    raise _refuse(path, "DQT Pq", pq, "16-bit quantisation tables are not decoded")
                if tq > 3 or q + 65 > len(body):
                    raise _refuse(path, "DQT Tq", tq, "a table 0 .. 3 of 64 entries is expected")
                nat = np.zeros(64, np.uint8)
                nat[list(_ZIGZAG)] = np.frombuffer(body[q + 1:q + 65], np.uint8)
                if nat.min() < 1:
                    raise _refuse(path, "DQT", 0, "a quantisation entry of 0")
                quant[tq] = nat
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                counts = list(body[q + 1:q + 17])
                total, code = sum(counts), 0
                if tc > 1 or th > 3 or len(counts) < 16:
                    raise _refuse(path, "DHT Tc/Th", (tc, th), "class 0 or 1 and table 0 .. 3 are expected")
                for length, c in enumerate(counts, 1):
                    code += c
                    if code > 1 << length:
                        raise _refuse(path, "DHT", f"{c} codes of length {length}", "the counts overflow the code space")
                    code <<= 1
                if total > 256 or q + 17 + total > len(body):
                    raise _refuse(path, "DHT", f"{total} values", "a table holds at most 256 values, all inside its segment")
                values = list(body[q + 17:q + 17 + total])
                if tc == 0 and values and max(values) > 15:
                    raise _refuse(path, "DHT", f"DC category {max(values)}", "a DC category is at most 15")
                tables[(tc, th)] = (counts, values)
                q += 17 + total
        elif m in _SOF:
            raise _refuse(path, f"SOF{m - 0xC0}", f"FF{m:02X}", f"{_SOF[m]} is not decoded; baseline SOF0 is")
        elif m in (0xC0, 0xC1):
            if sof is None and len(body) >= 6:
                p, y, x, nf = struct.unpack(">BHHB", body[:6])
                if p != 8:
                    raise _refuse(path, f"SOF{m - 0xC0} precision", p, "8-bit samples are decoded")
                if nf not in (1, 3) or len(body) < 6 + 3 * nf:
                    raise _refuse(path, f"SOF{m - 0xC0} Nf", nf, "1 or 3 components are decoded")
                if x < 1 or y < 1:
                    raise _refuse(path, f"SOF{m - 0xC0} size", (x, y), "width and height of at least 1 are expected")
                comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nf)]
                sof = (m, y, x, comps)
        elif m == 0xDD and len(body) >= 2:
            dri = struct.unpack(">H", body[:2])[0]
        elif m == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xE1 and body[:6] == b"Exif\0\0":
            orientation = _exif_orientation(body[6:])
        elif m == 0xDA:
            if sof is None:
                raise _refuse(path, "SOS", f"byte {pos}", "a scan in front of its frame header")
            ns = body[0] if body else 0
            if ns != len(sof[3]) or len(body) < 1 + 2 * ns + 3:
                raise _refuse(path, "SOS Ns", ns, f"several scans: one scan of all {len(sof[3])} components is decoded")
            scan = [(body[1 + 2 * c], body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(ns)]
            scan_off = pos + 2 + n
        pos += 2 + n
    _, height, width, comps = sof
    nf = len(comps)
    ids = [c[0] for c in comps]
    if [s[0] for s in scan] != ids:
        raise _refuse(path, "SOS Cs", [s[0] for s in scan], f"the frame's components {ids} in their order are expected")
    if nf == 3:
        # libjpeg's rule for three components
        if not jfif:
            if adobe is not None:
                if adobe != 1:
                    raise _refuse(path, "APP14 Adobe transform", adobe, "transform 1 (YCbCr) is decoded")
            elif ids != [1, 2, 3]:
                what = "RGB components" if bytes(ids) == b"RGB" else "components no rule reads as YCbCr"
                raise _refuse(path, "SOF component ids", ids if bytes(ids) != b"RGB" else "'R', 'G', 'B'", f"{what}; ids 1, 2, 3 are decoded")
        samp = [(c[1], c[2]) for c in comps]
        if samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise _refuse(path, "SOF sampling", samp, "luma (1,1), (2,1) or (2,2) with chroma (1,1) is decoded")
        hmax, vmax = samp[0]
    else:
        hmax = vmax = 1     # (a scan of one component is not interleaved: its MCU is one block whatever Hi, Vi say)
    for c in range(nf):
        if comps[c][3] not in quant:
            raise _refuse(path, "SOF Tq", comps[c][3], f"component {c} selects a quantisation table the file does not define")
        for cls, name, t in ((0, "Td", scan[c][1]), (1, "Ta", scan[c][2])):
            if t > 1 or (cls, t) not in tables or not tables[(cls, t)][1]:
                raise _refuse(path, f"SOS {name}", t, f"component {c} selects a Huffman table the file does not define (0 and 1 are decoded)")
    if dri < 1 and split is None:
        raise _refuse(path, "DRI", "none" if dri == 0 else dri,
                      "no restart interval: the scan is one serial walk, which the device decoder does not take")
    if dri > MAX_DRI and split is None:
        raise _refuse(path, "DRI", dri, f"a restart interval of more than {MAX_DRI} MCUs, the longest MCU row a JPEG can have: "
                                        "one wavefront walks an interval serially, and a picture in one piece is what is not decoded")
    # the intervals: FF followed by anything but 00
    body = data[scan_off:]
    ff = np.flatnonzero(body[:-1] == 0xFF) if len(body) > 1 else np.zeros(0, np.int64)
    nxt = body[ff + 1]
    cand, mk = ff[nxt != 0], nxt[nxt != 0]
    other = np.flatnonzero((mk < 0xD0) | (mk > 0xD7))
    if len(other) == 0:
        raise _refuse(path, "EOI", "none", "the file ends inside the scan")
    e = int(other[0])
    if mk[e] == 0xFF:
        raise _refuse(path, "fill byte", f"FF FF at byte {scan_off + int(cand[e])}", "fill bytes inside the scan are not decoded")
    if mk[e] != 0xD9:
        raise _refuse(path, f"marker FF{int(mk[e]):02X}", f"byte {scan_off + int(cand[e])}",
                      "several scans: a segment follows the first scan where EOI is expected")
    want = (0xD0 + np.arange(e) % 8).astype(np.uint8)
    wrong = np.flatnonzero(mk[:e] != want)
    if len(wrong):
        k = int(wrong[0])
        raise _refuse(path, f"RST{int(mk[k]) - 0xD0}", f"byte {scan_off + int(cand[k])}", f"restart markers out of sequence: RST{k % 8} is expected")
    n_mcus = -(-width // (8 * hmax)) * -(-height // (8 * vmax))
    to_split = split == "always" or (split == "needed" and (dri < 1 or dri > MAX_DRI))
    per = min(dri, n_mcus) if dri >= 1 else n_mcus      # (an interval longer than the picture is the picture)
    n_int = -(-n_mcus // per)
    if e + 1 != n_int:
        raise _refuse(path, "restart intervals", e + 1, f"{n_mcus} MCUs at DRI {dri if dri >= 1 else 'none'} make {n_int}")
    end = int(cand[e])
    if end >= 1 << 32:
        raise _refuse(path, "scan", end, "a scan of 4 GiB or more")
    offsets = np.empty(n_int + 1, np.uint32)
    offsets[0] = 0
    offsets[1:n_int] = cand[:e] + 2
    offsets[n_int] = end
    span = body[:max(end, 1)]
    d = _lib.JpegStruct()
    d.width, d.height, d.ncomp, d.hmax, d.vmax, d.dri, d.n_intervals = width, height, nf, hmax, vmax, per if to_split else dri, n_int
    for c in range(nf):
        d.tq[c], d.td[c], d.ta[c] = comps[c][3], scan[c][1], scan[c][2]
    for (cls, t), (counts, values) in tables.items():
        if t <= 1:
            for i, v in enumerate(counts):
                d.counts[2 * cls + t][i] = v
            for i, v in enumerate(values):
                d.values[2 * cls + t][i] = v
    for t in range(4):
        for i in range(64):
            d.quant[t][i] = int(quant[t][i]) if t in quant else 1
    return JpegFrame(path, (height, width), nf, (hmax, vmax), dri, span, offsets, d, orientation, mm, to_split)


def check_status(path, status):
    """ImageLoadError naming the file, the first flagged restart interval of `status` and its flags"""
    status = np.atleast_1d(np.asarray(status))
    bad = np.flatnonzero(status)
    if len(bad):
        k = int(bad[0])
        raise ImageLoadError(path, f"JPEG: restart interval {k} of {len(status)} did not decode "
                                   f"(status {int(status[k])}: {_lib.jpeg_flag_text(int(status[k]))})")


def _span(frame):
    return np.ascontiguousarray(frame.span)


def _split_opt(frame, max_rounds=None):
    o = _lib.JpegSplitStruct()
    o.sub_bytes, o.max_rounds = frame.split_options
    if max_rounds is not None:
        o.max_rounds = max_rounds
    return o


def coefficients(frame, device=0):
    """(per component its (rows of blocks, blocks a row, 64) int16 plane, the uint32 status words): the entropy kernel alone
    (jpeg_entropy, or the split decoder's passes where frame.split says so)"""
    _lib.require_device()
    n = _lib.C.c_size_t()
    _lib.check(_lib.load().mi_jpeg_coef_count(_lib.C.byref(frame.desc), _lib.C.byref(n)))
    coef = np.empty(n.value, np.int16)
    status = np.zeros(frame.n_intervals, np.uint32)
    span = _span(frame)
    if frame.split:
        _lib.check(_lib.load().mi_jpeg_split_coefficients(device, span.ctypes.data, span.nbytes, frame.offsets.ctypes.data,
                                                          _lib.C.byref(frame.desc), _lib.C.byref(_split_opt(frame)), coef.ctypes.data,
                                                          status.ctypes.data))
    else:
        _lib.check(_lib.load().mi_jpeg_coefficients(device, span.ctypes.data, span.nbytes, frame.offsets.ctypes.data,
                                                    _lib.C.byref(frame.desc), coef.ctypes.data, status.ctypes.data))
    out, at = [], 0
    for shape in frame.coef_shapes():
        k = shape[0] * shape[1] * 64
        out.append(coef[at:at + k].reshape(shape))
        at += k
    return out, status


def decode(frame, device=0, status=False):
    """The host form: upload, run, download, wait -> H x W x 3 BGR uint8.  A flagged interval raises ImageLoadError
    (check_status); with status=True nothing is raised and (frame, status words) is returned."""
    _lib.require_device()
    h, w = frame.shape
    out = np.empty((h, w, 3), np.uint8)
    st = np.zeros(frame.n_intervals, np.uint32)
    span = _span(frame)
    if frame.split:
        _lib.check(_lib.load().mi_jpeg_split_decode(device, span.ctypes.data, span.nbytes, frame.offsets.ctypes.data,
                                                    _lib.C.byref(frame.desc), _lib.C.byref(_split_opt(frame)), out.ctypes.data,
                                                    st.ctypes.data))
    else:
        _lib.check(_lib.load().mi_jpeg_decode(device, span.ctypes.data, span.nbytes, frame.offsets.ctypes.data, _lib.C.byref(frame.desc),
                                              out.ctypes.data, st.ctypes.data))
    if status:
        return out, st
    check_status(frame.path, st)
    return out


class Slot:
    """The device buffers one frame's decode needs -- span, offsets, status words, scratch -- grown as frames ask and kept
    from frame to frame.  `load` uploads and waits for the copy; `status` downloads the words of the last decode (wait for
    the kernels first)."""

    def __init__(self, device=0):
        self.device, self.buf, self.scratch = device, None, None
        self.n_intervals = 0

    def load(self, frame):
        span = _span(frame)
        self.off_at = (span.nbytes + 255) & ~255
        self.status_at = self.off_at + ((frame.offsets.nbytes + 255) & ~255)
        need = self.status_at + 4 * frame.n_intervals
        if self.buf is None or self.buf.nbytes < need:
            if self.buf is not None:
                self.buf.free()
            self.buf = _lib.DeviceBuffer(need, self.device)
        nb = _lib.C.c_size_t()
        if frame.split:     # (room for every round: a frame that reports UNSYNCED is decoded again in the same slot)
            _lib.check(_lib.load().mi_jpeg_split_scratch_bytes(_lib.C.byref(frame.desc), span.nbytes,
                                                               _lib.C.byref(_split_opt(frame, _lib.JPEG_SPLIT_ALL_ROUNDS)), _lib.C.byref(nb)))
        else:
            _lib.check(_lib.load().mi_jpeg_scratch_bytes(_lib.C.byref(frame.desc), _lib.C.byref(nb)))
        if self.scratch is None or self.scratch.nbytes < nb.value:
            if self.scratch is not None:
                self.scratch.free()
            self.scratch = _lib.DeviceBuffer(nb.value, self.device)
        self.buf.upload(span)
        self.buf.upload(frame.offsets, self.off_at)
        self.span_bytes, self.n_intervals = span.nbytes, frame.n_intervals

    def status(self):
        return self.buf.download((self.n_intervals,), np.uint32, self.status_at)

    def free(self):
        for b in (self.buf, self.scratch):
            if b is not None:
                b.free()
        self.buf = self.scratch = None


def decode_device(frame, dev_out, slot=None, device=0, stream=None, max_rounds=None, loaded=False):
    """Upload the frame's span into `slot` (a Slot; a new one when None) and enqueue the kernels on `stream`: `dev_out`
    (device pointer, H x W x 3 uint8) holds the BGR frame once they have run.  Does not wait for them.  Returns the slot: it
    owns the buffers the kernels read, and `slot.status()` gives the status words after a wait.  A frame with `split` set
    goes through the split decoder, with `max_rounds` in place of its own option where given; its status words may then
    hold JPEG_UNSYNCED (`settle`).  loaded: the slot holds this frame's span already."""
    _lib.require_device()
    slot = Slot(device) if slot is None else slot
    if not loaded:
        slot.load(frame)
    if frame.split:
        _lib.check(_lib.load().mi_jpeg_split_decode_device(device, stream, slot.buf.ptr, slot.span_bytes, slot.buf.ptr + slot.off_at,
                                                           _lib.C.byref(frame.desc), _lib.C.byref(_split_opt(frame, max_rounds)),
                                                           slot.scratch.ptr, slot.scratch.nbytes, dev_out, slot.buf.ptr + slot.status_at))
    else:
        _lib.check(_lib.load().mi_jpeg_decode_device(device, stream, slot.buf.ptr, slot.span_bytes, slot.buf.ptr + slot.off_at,
                                                     _lib.C.byref(frame.desc), slot.scratch.ptr, slot.scratch.nbytes, dev_out,
                                                     slot.buf.ptr + slot.status_at))
    return slot


def settle(frame, dev_out, slot, device=0):
    """After a wait for decode_device's kernels: the status words -- and where the split decoder says its rounds were too few
    (JPEG_UNSYNCED), the frame decoded once more from the slot with every round, waited for, and those words"""
    st = slot.status()
    if frame.split and (st & _lib.JPEG_UNSYNCED).any():
        decode_device(frame, dev_out, slot, device, None, _lib.JPEG_SPLIT_ALL_ROUNDS, loaded=True)
        _lib.check(_lib.load().mi_device_synchronize(device))
        st = slot.status()
    return st


def frames_device(paths, dev_out, device=0, split=None):
    """Read the n JPEG files (equal shape; `split` as in read), upload their spans and decode them side by side into `dev_out`
    (device pointer, n x H x W x 3 uint8): exactly what pipeline.align_and_stack_device(dev_frames, ...) takes, as
    dng.frames_device does for raw files.  Waits for the device; a flagged file raises ImageLoadError.  Returns (H, W, dtype)."""
    if len(paths) == 0:
        raise ValueError("no files")
    _lib.require_device()
    slots = [Slot(device), Slot(device)]
    pending = [None, None]
    first = None
    try:
        for i, p in enumerate(paths):
            frame = read(p, split)
            if first is None:
                first = frame
            elif frame.shape != first.shape:
                raise InvalidOptionError("paths", p, f"a {frame.shape} frame among {first.shape} ones")
            k = i & 1
            if pending[k] is not None:      # the slot's last decode: wait, then look at its status
                _lib.check(_lib.load().mi_device_synchronize(device))
                check_status(pending[k][0].path, settle(*pending[k], slots[k], device))
                pending[k] = None
            h, w = frame.shape
            decode_device(frame, dev_out + i * h * w * 3, slots[k], device)
            pending[k] = (frame, dev_out + i * h * w * 3)
        _lib.check(_lib.load().mi_device_synchronize(device))
        for k in (0, 1):
            if pending[k] is not None:
                check_status(pending[k][0].path, settle(*pending[k], slots[k], device))
    finally:
        _lib.load().mi_device_synchronize(device)
        for s in slots:
            s.free()
    return first.shape[0], first.shape[1], first.dtype


class Pusher:
    """The route of a stacker's `jpeg=` option: span up, kernels into one of two device BGR buffers used in alternation,
    then the handle's device push.  `push(frame, push_device, drain)` decodes one JpegFrame and hands the buffer's address to
    `push_device`; `drain` is the handle's own wait, called before a buffer is written again, so the upload of frame k + 1
    runs under the handle's kernels of frame k."""

    def __init__(self, device):
        self.device = device
        self.slots, self.bgr, self.k = [Slot(device), Slot(device)], [None, None], 0

    def push(self, frame, push_device, drain):
        k = self.k & 1
        h, w = frame.shape
        if self.bgr[k] is not None:
            drain()                         # what was pushed from this buffer two frames ago has been read
        if self.bgr[k] is None or self.bgr[k].nbytes < h * w * 3:
            if self.bgr[k] is not None:
                self.bgr[k].free()
            self.bgr[k] = _lib.DeviceBuffer(h * w * 3, self.device)
        slot = decode_device(frame, self.bgr[k].ptr, self.slots[k], self.device)
        _lib.check(_lib.load().mi_device_synchronize(self.device))       # the null stream's kernels, ahead of the handle's
        check_status(frame.path, settle(frame, self.bgr[k].ptr, slot, self.device))
        push_device(self.bgr[k].ptr)
        self.k += 1

    def close(self):
        for b in self.bgr:
            if b is not None:
                b.free()
        for s in self.slots:
            s.free()
        self.bgr = [None, None]
