"""The depth-selected composite: every pixel taken from the frame the depth map names (no reference counterpart).

A pyramid stacker's second rendering of the same stack: no Laplacian fusion, so no halos around strong edges and no amplified
noise -- the partner people brush into the pyramid image where that one shows halos (`Stroke(source="depth_composite")`).  One HIP
kernel does the work (csrc/kernels_composite.hpp, whose header is the specification; tests/depth_render_restatement.py restates
it in NumPy, bit for bit):

    d  = clamp(depth, 0, N - 1)                        NaN -> 0; float32, each operation rounded on its own
    'nearest':  out = frame[rint(d)]                   ties to even; samples are copied
    'linear':   k0 = floor(d), f = d - k0, k1 = min(k0 + 1, N - 1)
                out = frame[k0] + f * (frame[k1] - frame[k0])      rint and a clamp for the integer types; frame[k0] when f == 0

A call holds `count` consecutive frames from global index `first` and writes the pixels whose k0 it owns (first <= k0 <
first + count - 1, or k0 == N - 1 == first + count - 1), so calls that overlap by one frame render a stack of any length in
bounded memory: `composite` does that.  There is no CPU path: without a GPU or the library every entry point raises DeviceError.
"""
import ctypes as C

import numpy as np

from . import _lib
from .errors import BitDepthError, InvalidOptionError, ShapeError

INTERP = {"linear": 0, "nearest": 1}        # MI_COMPOSITE_LINEAR / MI_COMPOSITE_NEAREST
DTYPES = (np.uint8, np.uint16, np.float32)
SOURCE = "depth_composite"                  # the Stroke.source that names the composite


def check_options(interp="linear"):
    """Raise InvalidOptionError unless `interp` is 'linear' or 'nearest'; returns it"""
    if not isinstance(interp, str) or interp not in INTERP:
        raise InvalidOptionError("interp", interp, "one of " + ", ".join(repr(k) for k in INTERP))
    return interp


def check_chunk(first, count, n_frames):
    """Raise InvalidOptionError unless the frames first .. first + count - 1 are a chunk of a stack of `n_frames`"""
    for name, v in (("first", first), ("count", count), ("n_frames", n_frames)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise InvalidOptionError(name, v, "an integer")
    if n_frames < 1:
        raise InvalidOptionError("n_frames", n_frames, "a stack has at least one frame")
    if count < 1 or first < 0 or first + count > n_frames:
        raise InvalidOptionError("count", (first, count), f"the chunk leaves the stack's [0, {n_frames})")
    if count == 1 and n_frames > 1:
        raise InvalidOptionError("count", count, f"a chunk of a stack of {n_frames} frames holds at least 2 of them")


def _check_dtype(dtype):
    dt = np.dtype(dtype)
    if dt not in DTYPES:
        raise BitDepthError("uint8, uint16 or float32", dt)
    return dt


def composite_device(dev_frames, first, count, n_frames, dev_depth, dev_out, height, width, dtype, interp="linear", device=0,
                     stream=None):
    """One call of the kernel on data resident in HBM: `dev_frames` are the device addresses of the `count` frames with global
    indices first .. first + count - 1 (H x W x 3 of `dtype` each), `dev_depth` the H x W float32 plane, `dev_out` the output
    frame, of which only the pixels the chunk owns are written.  The frames and the plane are only read; `dev_out` is none of
    them.  Queued on `stream`, not waited for."""
    dt = _check_dtype(dtype)
    check_options(interp)
    check_chunk(first, count, n_frames)
    if height < 1 or width < 1:
        raise InvalidOptionError("frames", (height, width), "the composite is rendered from H x W x 3 frames")
    ptrs = [int(p) for p in dev_frames]
    if len(ptrs) != count:
        raise InvalidOptionError("dev_frames", len(ptrs), f"the chunk holds {count} frames")
    _lib.require_device()
    table = (C.c_void_p * count)(*ptrs)
    _lib.check(_lib.load().mi_depth_composite_device(int(device), stream, table, int(first), int(count), int(n_frames), dev_depth,
                                                     dev_out, int(height), int(width), _lib.DTYPE_CODE[dt], INTERP[interp]))


def _check_frame(frame, ref):
    a = np.asarray(frame)
    if ref is None:
        _check_dtype(a.dtype)
        if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise InvalidOptionError("frames", a.shape, "the composite is rendered from H x W x 3 frames")
    else:
        if a.dtype != ref.dtype:
            raise BitDepthError(ref.dtype, a.dtype)
        if a.shape != ref.shape:
            if a.ndim < 2:
                raise InvalidOptionError("frames", a.shape, "the composite is rendered from H x W x 3 frames")
            raise ShapeError(ref.shape, a.shape)
    return np.ascontiguousarray(a)


def default_resident(frame_bytes, device=0):
    """Frames a chunk holds by default: what a quarter of the free device memory takes, and at least 2"""
    free, _total = _lib.mem_info(device)
    return max(2, int(free // 4 // max(int(frame_bytes), 1)))


def composite(frames, depth, interp="linear", device=0, resident=None):
    """The composite of `frames` (a sequence of H x W x 3 uint8 / uint16 / float32 arrays of one shape and type, or any iterable
    that yields them in order) by `depth` (H x W, taken as float32 frame numbers).  Returns a new array of the frames' shape and
    type.

    The frames are uploaded in chunks of at most `resident` (default: `default_resident`) that overlap by one frame; the frame
    that ends a chunk stays on the device and starts the next one, and the reader is one frame ahead of the chunk, so neither the
    host nor the device ever holds the whole stack.  The stack's length need not be known in advance: a chunk that is not the
    last one is rendered as a chunk of a stack one frame longer than what has been read, which owns the same pixels."""
    check_options(interp)
    if resident is not None:
        if isinstance(resident, bool) or not isinstance(resident, (int, np.integer)) or resident < 2:
            raise InvalidOptionError("resident", resident, "a chunk holds at least 2 frames")
        resident = int(resident)
    depth = np.asarray(depth)
    if depth.ndim != 2 or depth.dtype.kind not in "fiu":
        raise InvalidOptionError("depth", depth.shape, "the depth map is an H x W plane of frame numbers")
    it = iter(frames)
    try:
        ahead = _check_frame(next(it), None)
    except StopIteration:
        raise ValueError("no frames") from None
    ref = ahead
    h, w = ref.shape[:2]
    if depth.shape != (h, w):
        raise InvalidOptionError("depth", depth.shape, f"the depth map is the frames' H x W plane ({h} x {w})")
    depth = np.ascontiguousarray(depth, np.float32)
    _lib.require_device()
    if resident is None:
        resident = default_resident(ref.nbytes, device)
    slots, dep, out = [], None, None        # slots: the chunk's device frames, in frame order
    try:
        dep = _lib.DeviceBuffer(depth.nbytes, device)
        dep.upload(depth)
        out = _lib.DeviceBuffer(ref.nbytes, device)
        first, held = 0, 0                  # global index of slots[0]; frames of the chunk already on the device
        while True:
            while held < resident and ahead is not None:
                if held == len(slots):
                    slots.append(_lib.DeviceBuffer(ref.nbytes, device))
                slots[held].upload(ahead)
                held += 1
                nxt = next(it, None)
                ahead = None if nxt is None else _check_frame(nxt, ref)
            is_last = ahead is None         # (a chunk that is not the last one leaves a frame for the next: no chunk of one frame)
            composite_device([b.ptr for b in slots[:held]], first, held, first + held + (0 if is_last else 1), dep.ptr, out.ptr,
                             h, w, ref.dtype, interp, device)
            _lib.check(_lib.load().mi_device_synchronize(int(device)))      # the slots are overwritten next
            if is_last:
                break
            slots.insert(0, slots.pop(held - 1))        # the chunk's last frame starts the next chunk where it lies
            first, held = first + held - 1, 1
        return out.download(ref.shape, ref.dtype)
    finally:
        for b in slots + [dep, out]:
            if b is not None:
                b.free()
