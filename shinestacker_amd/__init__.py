"""shinestacker_amd -- MI355X-native focus-stacking hot path behind shinestacker's
FocusStack / StackJob action API."""
from .errors import (FocusStackError, InvalidOptionError, ImageLoadError, ImageSaveError,  # noqa: F401
                     AlignmentError, BitDepthError, ShapeError, RunStopException, DeviceError)
from .defaults import constants  # noqa: F401
from .pyramid import BaseStackAlgo, PyramidStack  # noqa: F401
from .depth_map import DepthMapStack  # noqa: F401
from .actions import (StackJob, FocusStack, FocusStackBunch, CombinedActions, SubAction,  # noqa: F401
                      get_bunches)

from .align import AlignFrames, align_images  # noqa: F401,E402
from .balance import BalanceFrames  # noqa: F401,E402
from .vignetting import Vignetting  # noqa: F401,E402
from .noise_detection import MaskNoise, NoiseDetection  # noqa: F401,E402
from .denoise import denoise  # noqa: F401,E402
from .sharpen import unsharp_mask  # noqa: F401,E402
from .white_balance import white_balance_from_rgb  # noqa: F401,E402
from . import depth_out  # noqa: F401,E402
from . import stereo  # noqa: F401,E402
from . import retouch  # noqa: F401,E402
from . import depth_render  # noqa: F401,E402
from .retouch import Stroke  # noqa: F401,E402
from . import demosaic  # noqa: F401,E402
from .demosaic import Calibration, Cfa, Develop, calibrate, debayer, flat_gain, master_frame  # noqa: F401,E402
from . import lens  # noqa: F401,E402
from .lens import Lens, LensCorrection  # noqa: F401,E402
from . import dng  # noqa: F401,E402

__all__ = ["dng", "lens", "Lens", "LensCorrection", "AlignFrames", "BalanceFrames", "Vignetting", "MaskNoise", "NoiseDetection", "denoise", "unsharp_mask", "white_balance_from_rgb", "depth_out", "stereo", "retouch", "depth_render", "Stroke", "demosaic", "Cfa", "Develop", "debayer", "Calibration", "master_frame", "flat_gain", "calibrate", "align_images", "PyramidStack", "DepthMapStack", "BaseStackAlgo", "StackJob", "FocusStack", "FocusStackBunch",
           "CombinedActions", "SubAction", "get_bunches", "constants"]
