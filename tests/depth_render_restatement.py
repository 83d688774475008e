"""The depth-selected composite restated in NumPy from the specification in the header of csrc/kernels_composite.hpp: every
pixel taken from the frame the depth plane names.  float32 throughout, every operation rounded on its own (NumPy never fuses a
multiply with an add).  The GPU tests hold the kernel to this bit for bit."""
import numpy as np


def indices(depth, n_frames):
    """(d, k0, f, k1, k) of every pixel: the clamped depth, its floor, the fraction, the upper neighbour, the nearest frame"""
    d = np.array(depth, np.float32, copy=True)
    d[np.isnan(d)] = np.float32(0)
    d = np.minimum(np.maximum(d, np.float32(0)), np.float32(n_frames - 1)).astype(np.float32)
    k0 = np.floor(d).astype(np.int32)
    f = (d - k0.astype(np.float32)).astype(np.float32)
    k1 = np.minimum(k0 + 1, n_frames - 1).astype(np.int32)
    k = np.rint(d).astype(np.int32)         # ties to even
    return d, k0, f, k1, k


def owned(k0, first, count, n_frames):
    """the pixels a call over the frames first .. first + count - 1 writes"""
    last = first + count - 1
    return ((k0 >= first) & (k0 < last)) | ((k0 == n_frames - 1) & (last == n_frames - 1))


def composite_chunk(frames, first, n_frames, depth, out, interp="linear"):
    """One call: `frames` are the `count` frames with global indices first .. first + count - 1; the pixels the call owns are
    written into `out` in place, every other pixel is left alone"""
    assert interp in ("linear", "nearest")
    count = len(frames)
    assert count >= 1 and 0 <= first <= n_frames - count and (count >= 2 or n_frames == 1)
    st = np.stack([np.asarray(fr) for fr in frames])
    dt = st.dtype
    _, k0, f, k1, k = indices(depth, n_frames)
    own = owned(k0, first, count, n_frames)
    ys, xs = np.nonzero(own)
    if interp == "nearest":
        out[ys, xs] = st[k[ys, xs] - first, ys, xs]
        return out
    a = st[k0[ys, xs] - first, ys, xs]
    b = st[k1[ys, xs] - first, ys, xs]
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    ff = f[ys, xs][:, None]
    with np.errstate(all="ignore"):
        df = (fb - fa).astype(np.float32)
        m = (ff * df).astype(np.float32)
        v = (fa + m).astype(np.float32)
        if dt != np.float32:
            top = np.float32(np.iinfo(dt).max)
            v = np.minimum(np.maximum(np.rint(v), np.float32(0)), top)
        res = v.astype(dt)
    out[ys, xs] = np.where(ff == np.float32(0), a, res)      # f == 0: the sample itself, bit for bit
    return out


def composite(frames, depth, interp="linear"):
    """The whole stack in one call"""
    frames = [np.asarray(fr) for fr in frames]
    out = np.zeros_like(frames[0])
    return composite_chunk(frames, 0, len(frames), depth, out, interp)


def chunks(n_frames, size):
    """(first, count) of consecutive calls that hold at most `size` frames, overlap by one frame and cover [0, n_frames)"""
    if n_frames == 1:
        return [(0, 1)]
    assert size >= 2
    return [(first, min(size, n_frames - first)) for first in range(0, n_frames - 1, size - 1)]


def composite_chunked(frames, depth, size, interp="linear", fill=0):
    frames = [np.asarray(fr) for fr in frames]
    out = np.full_like(frames[0], fill)
    for first, count in chunks(len(frames), size):
        composite_chunk(frames[first:first + count], first, len(frames), depth, out, interp)
    return out
