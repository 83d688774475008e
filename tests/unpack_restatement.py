"""raw_unpack restated in NumPy: the definition the kernel (csrc/kernels_unpack.hpp) is held to, bit for bit.  As plain as
possible: one sample at a time, bit arithmetic on Python ints.

    span        the uploaded bytes (uint8); offsets[k] the start of segment k inside it
    segment     k = (ys // seg_h) * nsx + xs // seg_w for the stored site (ys, xs), nsx = ceil(image_w / seg_w); inside it the
                row ry = ys % seg_h and the column xt = xs % seg_w; a row takes ceil(seg_w * bits / 8) bytes and starts on a
                byte boundary (edge tiles are stored whole, so this holds for them too)
    sample      the `bits` bits from bit xt * bits of the row, most significant bit first: bit i of the row is bit 7 - i % 8
                of its byte i // 8.  16 bits: the two bytes in the file's order.  8 bits: the byte.
    then        v = table[min(v, len - 1)] with a table;  out = (v << shift) truncated to the dtype
"""
import numpy as np


def sample(span, row_start, xt, bits, big_endian):
    """the sample at column xt of the segment row that starts at byte row_start"""
    if bits == 8:
        return int(span[row_start + xt])
    if bits == 16:
        b0, b1 = int(span[row_start + 2 * xt]), int(span[row_start + 2 * xt + 1])
        return (b0 << 8 | b1) if big_endian else (b1 << 8 | b0)
    v = 0
    for i in range(xt * bits, xt * bits + bits):
        v = v << 1 | (int(span[row_start + i // 8]) >> (7 - i % 8)) & 1
    return v


def unpack(span, offsets, bits, big_endian, image_h, image_w, seg_h, seg_w, crop_y, crop_x, h, w, shift, table):
    """the cropped h x w mosaic (uint8 for 8 bits, uint16 otherwise)"""
    span = np.asarray(span, np.uint8)
    nsx = -(-image_w // seg_w)
    row_bytes = (seg_w * bits + 7) // 8
    dtype = np.uint8 if bits == 8 else np.uint16
    maxv = int(np.iinfo(dtype).max)
    out = np.zeros((h, w), dtype)
    for y in range(h):
        ys = y + crop_y
        for x in range(w):
            xs = x + crop_x
            k = (ys // seg_h) * nsx + xs // seg_w
            v = sample(span, int(offsets[k]) + (ys % seg_h) * row_bytes, xs % seg_w, bits, big_endian)
            if table is not None:
                v = int(table[min(v, len(table) - 1)])
            out[y, x] = (v << shift) & maxv
    return out


def unpack_layout(span, layout):
    """`unpack` for a shinestacker_amd.dng.RawLayout (only its fields are read)"""
    return unpack(span, layout.offsets, layout.bits, layout.big_endian, layout.image_height, layout.image_width, layout.seg_height,
                  layout.seg_width, layout.crop_y, layout.crop_x, layout.height, layout.width, layout.shift, layout.table)
