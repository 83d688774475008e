#!/usr/bin/env python3
"""The reference's `examples/stack-from-frames.fsp` project (align -> balance -> focus stack) as a
script on the MI355X path.  Same action graph, same parameter names as shinestacker's
StackJob / CombinedActions / AlignFrames / BalanceFrames / FocusStack; only the imports differ.

    python examples/stack_from_frames.py <working_dir> <input_subdir> [--no-align] [--vignetting] [--noise-map FOLDER] [--denoise N]
    python examples/stack_from_frames.py <working_dir> <input_subdir> --mosaic RGGB [--black B] [--gains R G1 G2 B]

`--noise-map FOLDER` and `--vignetting` build the reference's full graph: NoiseDetection over the frames of FOLDER (dark frames,
under the working directory) writes noise-map/hot_pixels.png, then MaskNoise and Vignetting run in front of AlignFrames -- the
reference's sub-action order MaskNoise, Vignetting, AlignFrames, BalanceFrames.  `--denoise N` (1-10) is FocusStack's
`denoise_amount`: the fused frame passes through the non-local-means filter before it is written.

`--mosaic PATTERN` (no reference counterpart) reads the single-channel 16-bit PNG / TIFF files of the input folder as raw Bayer
mosaics of that pattern: they are uploaded as they are -- a third of a developed frame's bytes -- demosaiced on the device and
fused (`PyramidStack.focus_stack_arrays(mosaic=Cfa(...))`); no alignment, the result goes to <working_dir>/stack/.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shinestacker_amd import (AlignFrames, BalanceFrames, CombinedActions, FocusStack, MaskNoise, NoiseDetection,  # noqa: E402
                              PyramidStack, StackJob, Vignetting)
from shinestacker_amd.align import ecc_estimator  # noqa: E402


def stack_mosaics(args):
    """the files of the input folder as raw mosaics, fused, written to <working_dir>/stack/stack_<first name>"""
    from shinestacker_amd import Cfa
    from shinestacker_amd.imageio import read_img, write_img
    folder = os.path.join(args.working_dir, args.input_subdir)
    names = sorted(n for n in os.listdir(folder) if n.split(".")[-1] in ("png", "tif", "tiff"))
    if not names:
        raise SystemExit(f"no PNG / TIFF files in {folder}")
    mosaics = []
    for n in names:
        img = read_img(os.path.join(folder, n))       # a single-channel file comes back with three equal channels
        if (img[..., 0] != img[..., 1]).any() or (img[..., 0] != img[..., 2]).any():
            raise SystemExit(f"{n} is a colour image, not a single-channel mosaic")
        mosaics.append(img[..., 0].copy())
    cfa = Cfa(args.mosaic, black=args.black, gains=args.gains)
    algo = PyramidStack()
    try:
        fused = algo.focus_stack_arrays(mosaics, mosaic=cfa)
    finally:
        algo.close()
    out = os.path.join(args.working_dir, "stack")
    os.makedirs(out, exist_ok=True)
    write_img(os.path.join(out, "stack_" + names[0]), fused)
    print("written:", sorted(os.listdir(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("working_dir")
    ap.add_argument("input_subdir")
    ap.add_argument("--no-align", action="store_true")
    ap.add_argument("--vignetting", action="store_true", help="correct the vignetting of every frame before it is aligned")
    ap.add_argument("--noise-map", metavar="FOLDER", help="map the hot pixels of the frames in FOLDER (relative to the working "
                    "directory) first, and mask them in every frame")
    ap.add_argument("--denoise", type=int, default=0, metavar="N", help="FocusStack(denoise_amount=N): denoise the result, "
                    "strength and template window N (1-10)")
    ap.add_argument("--mosaic", metavar="PATTERN", choices=("RGGB", "BGGR", "GRBG", "GBRG"),
                    help="the input files are single-channel raw Bayer mosaics of this pattern")
    ap.add_argument("--black", type=int, default=0, help="--mosaic: the sensor's black level")
    ap.add_argument("--gains", type=float, nargs=4, default=[1.0, 1.0, 1.0, 1.0], metavar="G",
                    help="--mosaic: the gains of the four cell positions, row-major (white balance, bit-depth scaling), each in [0, 16)")
    args = ap.parse_args()
    if args.mosaic:
        return stack_mosaics(args)
    job = StackJob("focus-stack", args.working_dir, input_path=args.input_subdir)
    stack_input = args.input_subdir
    if args.noise_map:
        job.add_action(NoiseDetection("noise-map", input_path=args.noise_map))
    if not args.no_align:
        pre = ([MaskNoise()] if args.noise_map else []) + ([Vignetting()] if args.vignetting else [])
        job.add_action(CombinedActions("align-and-balance",
                                       pre + [AlignFrames(estimator=ecc_estimator()),
                                              BalanceFrames(channel="RGB", corr_map="MATCH_HIST")],
                                       input_path=args.input_subdir, output_path="align"))
        stack_input = "align"
    job.add_action(FocusStack("stack", PyramidStack(), input_path=stack_input, output_path="stack",
                              prefix="stack_", denoise_amount=args.denoise))
    job.run()
    print("written:", sorted(os.listdir(os.path.join(args.working_dir, "stack"))))


if __name__ == "__main__":
    main()
