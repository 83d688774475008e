"""MaskNoise on the MI355X path (reference algorithms/noise_detection.py:145-198).

The sub-action reads a hot-pixel mask (an 8-bit gray image file, non-zero = hot) once and replaces, in every frame and
every channel, each hot pixel by the mean or the median of the non-zero values of the uncorrected channel in a
`kernel_size` x `kernel_size` window (`mi_mask_noise_device`, csrc/kernels_prestack.hpp: one thread per hot pixel and
channel, integer arithmetic that equals the reference's float mean / median after its truncating assignment).

Same class, constructor arguments, messages and exceptions as the reference; `run_frame_device` is the same step for a
frame that lives in HBM.

`NoiseDetection` (noise_detection.py:21-143) is the action that PRODUCES the mask: the mean of the frames of one or several
folders (`mi_frame_accumulate_device`: exact uint32 sums), then in one launch mean -> Gaussian blur -> absolute difference ->
per-channel thresholds -> OR and the four counts (`mi_hot_pixel_map_device`), written as an 8-bit gray PNG.
Deviations from the reference, all stated in INTEGRATION.md: 16-bit frames raise BitDepthError (the reference casts a mean
above 255 to uint8, which is undefined); `blur_size` 3, 5 and 7 only; the files of a folder are taken in sorted order (the
reference's os.walk order is arbitrary; only the `max_frames` cut depends on it).
"""
import logging
import os

import numpy as np

from . import _lib
from .actions import ActionBase, FrameDirectory, SubAction, _join, _require_dir
from .defaults import constants
from .errors import BitDepthError, ImageLoadError, InvalidOptionError, RunStopException, ShapeError
from .imageio import read_img, validate_image

MAX_NOISY_PIXELS = 1000

_METHOD_CODE = {constants.INTERPOLATE_MEAN: 0, constants.INTERPOLATE_MEDIAN: 1}


def read_mask(path):
    """The mask file as an H x W uint8 array, or None when it cannot be decoded.  With OpenCV importable this is
    cv2.imread(path, cv2.IMREAD_GRAYSCALE).  Without it the file is decoded with Pillow: an 8-bit gray file (what
    NoiseDetection writes) comes back as it is; for any other format (16-bit, palette, colour, with or without alpha) a pixel
    is 255 where any colour sample of the UNDECODED image is non-zero and 0 elsewhere -- only zero / non-zero matters to
    MaskNoise, and a gray conversion could round a small non-zero sample to zero."""
    try:
        import cv2
        return cv2.imread(path, cv2.IMREAD_GRAYSCALE)
    except ImportError:
        pass
    try:
        from PIL import Image
        with Image.open(path) as im:
            if im.mode == "L":
                return np.ascontiguousarray(np.asarray(im, dtype=np.uint8))
            if im.mode in ("P", "PA", "1"):
                im = im.convert("RGBA" if "transparency" in im.info or im.mode == "PA" else "RGB")
            a = np.asarray(im)
            if a.ndim == 3:
                colour = a[..., :-1] if im.mode in ("LA", "RGBA", "La", "RGBa") else a
                hot = (colour != 0).any(axis=2)
            else:
                hot = a != 0
            return np.ascontiguousarray(hot.astype(np.uint8) * 255)
    except Exception:  # noqa: BLE001  cv2.imread returns None on undecodable files
        return None


class MaskNoise(SubAction):
    """Sub-action of CombinedActions (noise_detection.py:145-198)."""

    def __init__(self, noise_mask=constants.DEFAULT_NOISE_MAP_FILENAME, kernel_size=constants.DEFAULT_MN_KERNEL_SIZE,
                 method=constants.INTERPOLATE_MEAN, **kwargs):
        self.device = kwargs.pop('device', 0)
        super().__init__(**kwargs)
        if method not in constants.VALID_INTERPOLATE:
            raise InvalidOptionError("method", method, f"valid values are {sorted(constants.VALID_INTERPOLATE)}")
        if not isinstance(kernel_size, (int, np.integer)) or kernel_size < 1 or kernel_size % 2 == 0:
            raise InvalidOptionError("kernel_size", kernel_size, "must be an odd integer >= 1")
        self.noise_mask = noise_mask if noise_mask != '' else constants.DEFAULT_NOISE_MAP_FILENAME
        self.kernel_size = int(kernel_size)
        self.ks2 = self.kernel_size // 2
        self.ks2_1 = self.ks2 + 1
        self.method = method
        self.process = None
        self.noise_mask_img = None
        self._coords = None      # host (n, 2) int32 (y, x), np.argwhere order
        self._dev = None         # device: coordinates, then the staging values

    def begin(self, process):
        self.process = process
        f = getattr(process, "sub_message_r", None)
        self.load(f"{process.working_path}/{self.noise_mask}", f)

    def load(self, path, message=None):
        """Read the mask file at `path` (noise_detection.py:158-169: ImageLoadError when it is missing or undecodable)."""
        if not os.path.exists(path):
            raise ImageLoadError(path, "file not found.")
        if message is not None:
            message(f': reading noisy pixel mask file: {self.noise_mask}')
        self.set_mask(read_mask(path), path)

    def set_mask(self, mask, path=""):
        """Take the mask as an array (what `begin` does with the file it read)."""
        if mask is None:
            raise ImageLoadError(path, f"failed to load image file {self.noise_mask}.")
        self.noise_mask_img = np.asarray(mask)
        self._coords = np.ascontiguousarray(np.argwhere(self.noise_mask_img > 0), dtype=np.int32)
        self._free()

    def _free(self):
        if self._dev is not None:
            self._dev.free()
            self._dev = None

    def _check(self, height, width):
        n = self._coords.shape[0]
        if n > MAX_NOISY_PIXELS:   # noise_detection.py:185-186, raised per frame as there
            raise RuntimeError(f"Noise map contains too many hot pixels: {n}")
        if self.noise_mask_img.shape[:2] != (height, width):
            raise ShapeError((height, width), self.noise_mask_img.shape)
        return n

    def _upload(self, height, width):
        n = self._check(height, width)
        if self._dev is None and n > 0:
            self._dev = _lib.DeviceBuffer(n * 8 + n * 12, self.device)   # n (y, x) int32 pairs | n x 3 uint32
            self._dev.upload(self._coords)
        return n

    def run_frame_device(self, _idx, dev_img, height, width, dtype, stream=None, dev_dst=None):
        """run_frame for a frame resident in HBM: in place, or into `dev_dst`.  Enqueued on `stream`, no synchronisation."""
        n = self._upload(height, width)
        base = self._dev.ptr if n else None
        _lib.check(_lib.load().mi_mask_noise_device(self.device, stream, dev_img, dev_img if dev_dst is None else dev_dst,
                                                    int(height), int(width), _lib.DTYPE_CODE[np.dtype(dtype)], base, n,
                                                    self.kernel_size, _METHOD_CODE[self.method], base + 8 * n if n else None))

    def run_frame(self, _idx, _ref_idx, image):
        f = getattr(self.process, "sub_message_r", None)
        if f is not None:
            f(': mask noisy pixels')
        a = np.ascontiguousarray(image)
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype not in (np.uint8, np.uint16):
            raise ValueError("expected an H x W x 3 uint8/uint16 BGR frame")
        self._check(a.shape[0], a.shape[1])
        _lib.require_device()
        buf = _lib.DeviceBuffer(a.nbytes, self.device)
        try:
            buf.upload(a)
            self.run_frame_device(_idx, buf.ptr, a.shape[0], a.shape[1], a.dtype)
            _lib.check(_lib.load().mi_device_synchronize(self.device))
            return buf.download(a.shape, a.dtype)
        finally:
            buf.free()

    def end(self):
        self._free()


def write_mask(path, mask):
    """cv2.imwrite(path, mask) for an H x W uint8 image: an 8-bit gray PNG"""
    try:
        import cv2
        cv2.imwrite(path, mask)
    except ImportError:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(mask, dtype=np.uint8)).save(path)


class FrameMultiDirectory(FrameDirectory):
    """stack_framework.py:133-188: `input_path` is one folder or a list of folders under the working path; the file list
    holds paths relative to the working path, folder by folder, each folder's files in sorted order."""

    def folder_list_str(self):
        dirs = [self.input_full_path] if isinstance(self.input_full_path, str) else list(self.input_full_path)
        rel = ", ".join(d.replace(self.working_path, '').lstrip('/') for d in dirs)
        return "folder" + ('s' if len(dirs) > 1 and not isinstance(self.input_full_path, str) else '') + f": {rel}"

    def folder_filelist(self):
        if isinstance(self.input_full_path, str):
            dirs, paths = [self.input_full_path], [self.input_path]
        elif hasattr(self.input_full_path, "__len__"):
            dirs, paths = self.input_full_path, self.input_path
        else:
            raise RuntimeError("input_full_path option must contain a path or an array of paths")
        files = []
        for d, p in zip(dirs, paths):
            for _dirpath, _, names in os.walk(d):
                found = sorted(p + "/" + n for n in names if os.path.splitext(n)[-1][1:].lower() in constants.EXTENSIONS)
                if self.reverse_order:
                    found.reverse()
                if self.resample > 1:
                    found = found[0::self.resample]
                files += found
            if len(files) == 0:
                self.print_message(f"input folder {p} does not contain any image", level=logging.WARNING)
        return files

    def init(self, job, _working_path=''):
        many = not isinstance(self.input_path, str) and hasattr(self.input_path, "__len__")
        folders = list(self.input_path) if many else None
        if many:
            self.input_path = folders[0]       # init_paths checks one folder; the list is put back below
        self.init_paths(job)
        if many:
            self.input_path = folders
            self.input_full_path = [_join(self.working_path, f) for f in folders]
            for d in self.input_full_path:
                _require_dir(d)


class NoiseDetection(ActionBase, FrameMultiDirectory):
    """The job action that maps hot pixels (noise_detection.py:48-143)."""

    BATCH = 8   # frames added per launch

    def __init__(self, name="noise-map", enabled=True, **kwargs):
        self.device = kwargs.pop('device', 0)
        FrameMultiDirectory.__init__(self, name, **kwargs)
        ActionBase.__init__(self, name, enabled)
        self.max_frames = kwargs.get('max_frames', -1)
        self.blur_size = kwargs.get('blur_size', constants.DEFAULT_BLUR_SIZE)
        self.file_name = kwargs.get('file_name', constants.DEFAULT_NOISE_MAP_FILENAME)
        if self.file_name == '':
            self.file_name = constants.DEFAULT_NOISE_MAP_FILENAME
        self.channel_thresholds = kwargs.get('channel_thresholds', constants.DEFAULT_CHANNEL_THRESHOLDS)
        self.plot_range = kwargs.get('plot_range', constants.DEFAULT_NOISE_PLOT_RANGE)
        self.plot_histograms = kwargs.get('plot_histograms', False)
        if self.blur_size not in (3, 5, 7):
            raise InvalidOptionError("blur_size", self.blur_size, "3, 5 and 7 are implemented (OpenCV's fixed small kernels)")
        self.mean_img = self.hot_rgb = self.hot_counts = None
        self._sum = self._stage = None

    def progress(self, i):
        self.callback('after_step', self.id, self.name, i)

    def _step_done(self, i):
        self.progress(i)
        if self.callback('check_running', self.id, self.name) is False:
            raise RunStopException(self.name)

    # -- the two device steps (the host loop around them is tested without a GPU by replacing them)
    def _device_add(self, frames):
        """add a batch of equal-shaped uint8 frames into the device sum image (created on the first call)"""
        lib = _lib.load()
        slot = frames[0].size
        if self._sum is None:
            _lib.require_device()
            self._sum = _lib.DeviceBuffer(slot * 4, self.device)
            self._sum.upload(np.zeros(slot, np.uint32))
            self._stage = _lib.DeviceBuffer(slot * self.BATCH, self.device)
        step = len(frames) if slot % 4 == 0 else 1     # frames after the first of a launch must start on a dword
        for k0 in range(0, len(frames), step):
            part = frames[k0:k0 + step]
            for k, img in enumerate(part):
                self._stage.upload(img, k * slot)
            _lib.check(lib.mi_frame_accumulate_device(self.device, None, self._stage.ptr, len(part), slot, self._sum.ptr))
            _lib.check(lib.mi_device_synchronize(self.device))   # the staging buffer is refilled next

    def _device_map(self, counter, shape):
        """(mean image, hot map, [rgb, channel 0, 1, 2] counts) from the device sum image"""
        import ctypes as C
        h, w = shape[:2]
        mean, hot, scratch = (_lib.DeviceBuffer(h * w * 3, self.device), _lib.DeviceBuffer(h * w, self.device),
                              _lib.DeviceBuffer(16, self.device))
        try:
            counts = np.zeros(4, np.uint32)
            th = (C.c_int * 3)(*[int(t) for t in self.channel_thresholds])
            _lib.check(_lib.load().mi_hot_pixel_map_device(self.device, None, self._sum.ptr, counter, h, w, int(self.blur_size), th,
                                                           mean.ptr, hot.ptr, scratch.ptr, counts.ctypes.data))
            return mean.download((h, w, 3), np.uint8), hot.download((h, w), np.uint8), [int(c) for c in counts]
        finally:
            for b in (mean, hot, scratch):
                b.free()

    def _release(self):
        for b in (self._sum, self._stage):
            if b is not None:
                b.free()
        self._sum = self._stage = None

    def accumulate(self, in_paths):
        """noise_detection.py:21-45 with the sum on the GPU: (frames added, frame shape).  The loop stops when
        i > max_frames, i.e. max_frames + 1 frames are averaged while step_counts announced min(n, max_frames) -- the
        reference's own off-by-one, kept."""
        shape = dtype = None
        pending, counter = [], 0
        for i, path in enumerate(in_paths):
            if 1 <= self.max_frames < i:
                break
            self.print_message_r(f"reading frame: {path.split('/')[-1]}")
            if not os.path.exists(path):
                import errno
                raise FileNotFoundError(errno.ENOENT, os.strerror(errno.ENOENT), path)
            img = read_img(path)
            if shape is None:
                if img is None:
                    raise RuntimeError("Image is None")
                if img.dtype != np.uint8:
                    raise BitDepthError(np.dtype(np.uint8), img.dtype)
                shape, dtype = img.shape, img.dtype
            else:
                validate_image(img, shape, dtype)
            if counter + 1 >= 1 << 24:
                raise OverflowError("more than 2^24 frames: the uint32 sums would overflow")
            pending.append(np.ascontiguousarray(img))
            counter += 1
            if len(pending) == self.BATCH:
                self._device_add(pending)
                pending = []
            self._step_done(i)
        if pending:
            self._device_add(pending)
        return counter, shape

    def run_core(self):
        self.print_message(f"map noisy pixels from frames in {self.folder_list_str()}")
        files = self.folder_filelist()
        in_paths = [self.working_path + "/" + f for f in files]
        n_frames = min(len(in_paths), self.max_frames) if self.max_frames > 0 else len(in_paths)
        self.callback('step_counts', self.id, self.name, n_frames)
        try:
            counter, shape = self.accumulate(in_paths)
            if counter == 0:
                raise RuntimeError("Mean image is None")
            self.mean_img, self.hot_rgb, self.hot_counts = self._device_map(counter, shape)
        finally:
            self._release()
        self.print_message("hot pixels: " + ", ".join(f"{ch}: {c}" for ch, c in zip(['rgb', *constants.RGB_LABELS], self.hot_counts)))
        path = "/".join(self.file_name.split("/")[:-1])
        if not os.path.exists(f"{self.working_path}/{path}"):
            self.print_message(f"create directory: {path}")
            os.mkdir(f"{self.working_path}/{path}")
        self.print_message(f"writing hot pixels map file: {self.file_name}")
        write_mask(f"{self.working_path}/{self.file_name}", self.hot_rgb)
        if self.plot_histograms:
            self._plot_histograms()

    def _plot_histograms(self):
        """the thresholds in use and the hot pixels they gave, over plot_range widened to hold them (the reference draws
        the count against every threshold of the range; here only the thresholds in use are evaluated)"""
        from .vignetting import _pyplot, _save_plot
        plt = _pyplot()
        if plt is None:
            return
        lo = min(self.plot_range[0], min(self.channel_thresholds) - 1)
        hi = max(self.plot_range[1], max(self.channel_thresholds) + 1)
        fig, ax = plt.subplots(figsize=(10, 5))
        for c, label in enumerate(constants.RGB_LABELS):
            ax.plot([self.channel_thresholds[c]] * 2, [0, self.hot_counts[1 + c]], color=label, linestyle="--",
                    label=f"{label}: {self.hot_counts[1 + c]}")
        ax.set(xlabel="threshold", ylabel="# of hot pixels", xlim=(lo, hi))
        ax.set_ylim(bottom=0)
        ax.legend()
        plot_path = f"{self.working_path}/{self.plot_path}/{self.name}-hot-pixels.pdf"
        _save_plot(plt, plot_path)
        self.callback('save_plot', self.id, f"{self.name}: noise", plot_path)
