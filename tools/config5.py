#!/usr/bin/env python3
"""BASELINE config 5 on one GPU at reduced length: 16-bit 50 MP frames in HOST memory, stacked in
bunches (FocusStackBunch geometry: frames=10, overlap=2, stack.py:61-64) through the pinned asynchronous
upload path of mi_stack_push_frame -- PCIe, the bounce copy and the kernels overlap.  One stacker handle
serves every bunch (reset between bunches), as FocusStackBunch does.

Several GPUs (SURVEY 8(e) bunch mode, no collective in the data path): start it with
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/config5.py
Every rank fuses a contiguous block of the bunches on GPU LOCAL_RANK (actions.shard_steps, what
FocusStackBunch(shard='env') does); a gloo group is used for the two barriers and the max-over-ranks time only."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def two_stage(args):
    """config 5 is H2D-bound -- report OVERLAP EFFICIENCY = max(upload, compute) / wall:
      upload_s   the pushed bytes at this box's own pinned hipMemcpy rate (measured here: one 50 MP frame, 5 copies);
      compute_s  stage 1 with the same bunches taken from frames RESIDENT in HBM (no PCIe at all);
      wall_s     stage 1 as it runs: frames in host memory, upload + kernels overlapped.
    `--pinned` (default): the host frames lie in pinned memory (mi_host_alloc -- what a decoder writing into
    `_lib.host_alloc` arrays gives) and are uploaded without the bounce copy; `--pageable`: ordinary NumPy arrays through the
    three pinned bounce buffers and the copy-thread pool.
    `--mosaic`: stage 1 once more in the same process, from the RGGB mosaics of the same frames (`mi_stack_push_mosaic`: a third
    of the bytes over the link, demosaiced on the device behind the upload); the result line carries both stage-1 times, both
    byte counts and the stage-1 time of the resident BGR frames (`compute_s`) under "mosaic".
    `--develop` (with `--mosaic`): stage 1 a third time, the mosaics developed on the device (`mi_stack_push_mosaic_developed`:
    camera matrix, sRGB curve, 10 000 defect sites), then the plain mosaic run again; the times sit beside each other under
    "mosaic".
    `--packed BITS` (with `--mosaic`): stage 1 from packed spans of the same frames (`mi_stack_push_packed`: BITS / 16 of the
    mosaic's bytes over the link, unpacked on the device), in turns with the mosaic run on the same samples.
    `--ljpeg` (with `--mosaic --packed BITS`): stage 1 a further time from the same samples as lossless-JPEG spans
    (`mi_stack_push_ljpeg`: 256 x 256 tiles, two components, predictor 1, written by tools/ljpeg_encode.py; decoded on the device
    by raw_ljpeg), in turns with the packed and the mosaic runs; the handles' decode status is asserted to be 0.
    `--split` (with `--ljpeg`): the compressed stage 1 once more with the split path set on the handles (decode inside a
    segment), in turns with the serial kernel on the same spans.
    `--sitecorr` (with `--mosaic --packed BITS`): the packed stage 1 with site corrections (dng.SiteCorrections: black deltas
    and four 17 x 13 gain maps) set on every stage-1 handle, in turns with the packed run without them.
    `--calibrate` (with `--mosaic`): stage 1 from the mosaics with a `Calibration` (a master dark and a master flat; the gain
    table is built on the device before the clock starts) and without, three runs of each in turns, so that the two are
    compared inside one process and the spread from run to run shows; every time is listed under "mosaic"."""
    from shinestacker_amd import _lib as L
    from shinestacker_amd.pipeline import bunches_then_stack
    N, H, W = args.frames, args.height, args.width
    per = H * W * 3 * 2
    ndist = 8   # distinct host frames, cycled (a real job decodes files here; 130 distinct 50 MP frames are 39 GB)
    buf = L.DeviceBuffer(per * ndist)
    L.synth_frames_device(buf.ptr, np.uint16, H, W, 0, ndist, ndist)
    host = []
    for i in range(ndist):
        fr = buf.download((H, W, 3), np.uint16, offset=i * per)
        if not args.pageable:
            pin = L.host_alloc((H, W, 3), np.uint16)
            pin[...] = fr
            fr = pin
        host.append(fr)
    # this box's pinned host-to-device rate: the ceiling of any upload path
    pin0 = host[0] if not args.pageable else L.host_alloc((H, W, 3), np.uint16)
    # ... measured through the library's own copy stream (asynchronous copies out of pinned memory, ten frames back to back,
    # the best of three rounds; a synchronous hipMemcpy read 29 or 57 GB/s from run to run on the same box)
    cal = L.Stack(H, W, in_dtype=np.uint16, out_dtype=np.uint16)
    rates = []
    for _ in range(3):
        cal.reset()
        t0 = time.perf_counter()
        for _k in range(10):
            cal.push_frame(pin0, zero_copy=True)
        cal.wait_uploads(0)
        rates.append(10 * per / (time.perf_counter() - t0))
    cal.close()
    pinned_rate = max(rates)
    out = L.DeviceBuffer(per)
    nst = 2 if args.one_handle else 3     # stage 1 alternates between two handles unless --one-handle (the round-3 flow)
    stacks = tuple(L.Stack(H, W, in_dtype=np.uint16, out_dtype=np.uint16) for _ in range(nst))

    # the buffer of the bunch results is made once, like the handles (a job of many stacks keeps it): allocating and freeing
    # it costs ~50 ms per GB, 2 s for the 38 GB of a 1024-frame job, and is reported separately
    from shinestacker_amd.actions import get_bunches
    nbunch = len(get_bunches(list(range(N)), 10, 2))
    t0 = time.perf_counter()
    results = L.DeviceBuffer(per * nbunch)
    L.check(L.load().mi_device_synchronize(0))
    results_alloc_s = time.perf_counter() - t0

    def run():
        info = {}
        _, bunches = bunches_then_stack(lambda i: host[i % ndist], N, H, W, np.uint16, out_dev=out.ptr,
                                        stacks=stacks, results_buf=results, info=info, zero_copy=not args.pageable)
        return bunches, info["stage1_s"], info["stage2_s"]
    run()
    bunches, s1, s2 = run()
    pushed = sum(len(b) for b in bunches)
    # stage 1 with the frames resident: the compute side alone
    st = stacks[0]

    def resident():
        for b in bunches:
            st.reset()
            for i in b:
                st.push_frames_device(buf.ptr + (i % ndist) * per, 1, per)
            st.finish_device(out.ptr)
        st.sync()
    resident()
    t0 = time.perf_counter()
    resident()
    compute_s = time.perf_counter() - t0
    upload_s = pushed * per / pinned_rate
    extra = {}
    if args.mosaic:
        from shinestacker_amd.demosaic import Cfa, mosaic_of
        cfa = Cfa("RGGB")
        mos = []
        for fr in host:
            m = mosaic_of(fr, cfa.pattern)
            if not args.pageable:
                pin = L.host_alloc((H, W), np.uint16)
                pin[...] = m
                m = pin
            mos.append(m)

        def run_mosaic():
            info = {}
            bunches_then_stack(lambda i: mos[i % ndist], N, H, W, np.uint16, out_dev=out.ptr, stacks=stacks, results_buf=results,
                               info=info, zero_copy=not args.pageable, mosaic=cfa)
            return info["stage1_s"], info["stage2_s"]
        run_mosaic()
        m1, m2 = run_mosaic()
        developed = {}
        if args.develop:
            # stage 1 once more, developed: a camera matrix, the sRGB curve and 10 000 defect sites ride on the demosaic; then
            # the plain mosaic run again, so that the two are compared inside one process and in both orders
            from shinestacker_amd.demosaic import Develop
            rng = np.random.default_rng(5)
            sites = np.stack([rng.integers(0, H, 10000), rng.integers(0, W, 10000)], axis=1)
            with Develop(matrix=[[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [0.05, -0.55, 1.5]], tone="srgb", defects=sites) as dv:
                def run_developed():
                    info = {}
                    bunches_then_stack(lambda i: mos[i % ndist], N, H, W, np.uint16, out_dev=out.ptr, stacks=stacks,
                                       results_buf=results, info=info, zero_copy=not args.pageable, mosaic=cfa, develop=dv)
                    return info["stage1_s"], info["stage2_s"]
                run_developed()
                d1, d2 = run_developed()
                for s_ in stacks:
                    s_.sync()
            m1b, _ = run_mosaic()
            developed = {"developed_stage1_seconds": d1, "developed_stage2_seconds": d2, "stage1_seconds_again": m1b,
                         "developed_over_plain_stage1": d1 / m1, "defect_sites": len(dv.sites((H, W)))}
        if args.calibrate:
            from shinestacker_amd.demosaic import Calibration
            rng = np.random.default_rng(7)
            yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
            fall = 1.0 - 0.7 * (((yy - H / 2) / (H / 2)) ** 2 + ((xx - W / 2) / (W / 2)) ** 2) / 2
            del yy, xx
            flat = (40000.0 * fall).astype(np.uint16)
            del fall
            dark = rng.integers(0, 512, size=(H, W)).astype(np.uint16)
            with Calibration(dark=dark, flat=flat) as cb:
                cb.prepared((H, W), np.uint16, cfa)      # the tables are built and uploaded once per session: not timed

                def run_calibrated():
                    info = {}
                    bunches_then_stack(lambda i: mos[i % ndist], N, H, W, np.uint16, out_dev=out.ptr, stacks=stacks,
                                       results_buf=results, info=info, zero_copy=not args.pageable, mosaic=cfa, calibration=cb)
                    return info["stage1_s"]
                run_calibrated()
                with_c, without = [], []
                for _ in range(3):
                    with_c.append(run_calibrated())
                    without.append(run_mosaic()[0])
                for s_ in stacks:
                    s_.sync()
            developed.update({"calibrated_stage1_seconds": with_c, "plain_stage1_seconds_in_turns": without,
                              "calibrated_over_plain_stage1": float(np.median(with_c) / np.median(without)),
                              "plain_stage1_spread": float((max(without) - min(without)) / np.median(without))})
        if args.packed:
            # stage 1 from packed spans of the SAME frames (the mosaics' top `--packed` bits, stored as a raw file stores them:
            # strips of 64 rows, rows packed most significant bit first), in turns with the mosaic run.  The mosaics pushed
            # beside them are the unpacked spans, so both runs fuse the same samples.
            from shinestacker_amd import dng
            bits = args.packed
            rowb = (W * bits + 7) // 8
            rps = 64
            offsets = np.arange(-(-H // rps), dtype=np.uint32) * np.uint32(rps * rowb)
            lay = dng.RawLayout(bits, False, H, W, False, rps, W, offsets, shift=16 - bits)
            pk, same, lj = [], [], []
            if args.ljpeg:
                sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
                import ljpeg_encode
            for m in mos:
                v = (np.asarray(m) >> (16 - bits)).astype(np.uint16)
                if args.ljpeg:
                    cspan, segs = ljpeg_encode.encode_frame(v, bits, 256, 256, True)
                    if not args.pageable:
                        pin = L.host_alloc(cspan.shape, np.uint8)
                        pin[...] = cspan
                        cspan = pin
                    clay = dng.RawLayout(bits, False, H, W, True, 256, 256, np.zeros(len(segs), np.uint32), shift=16 - bits, compression=7,
                                         segments=segs)
                    lj.append(dng.DngFrame("<memory>", clay, cspan, cfa, None, None, 1, ()))
                if bits == 16:
                    span = v.view(np.uint8).reshape(-1)
                elif bits == 12 and W % 2 == 0:      # two samples are three bytes
                    a_, b_ = v[:, 0::2], v[:, 1::2]
                    span = np.stack([a_ >> 4, (a_ & 15) << 4 | b_ >> 8, b_ & 255], axis=2).astype(np.uint8).reshape(-1)
                else:
                    bit = np.unpackbits(v.byteswap().view(np.uint8).reshape(H, W, 2), axis=2)[:, :, 16 - bits:].reshape(H, W * bits)
                    bit = np.concatenate([bit, np.zeros((H, rowb * 8 - W * bits), np.uint8)], axis=1)
                    span = np.packbits(bit, axis=1).reshape(-1)
                    del bit
                if not args.pageable:
                    pin = L.host_alloc(span.shape, np.uint8)
                    pin[...] = span
                    span = pin
                pk.append(dng.DngFrame("<memory>", lay, span, cfa, None, None, 1, ()))
                low = (v << (16 - bits)).astype(np.uint16)
                if not args.pageable:
                    pin = L.host_alloc((H, W), np.uint16)
                    pin[...] = low
                    low = pin
                same.append(low)

            def run_packed():
                info = {}
                bunches_then_stack(lambda i: pk[i % ndist], N, H, W, np.uint16, out_dev=out.ptr, stacks=stacks, results_buf=results,
                                   info=info, zero_copy=not args.pageable, packed=True)
                return info["stage1_s"]

            def run_same():
                info = {}
                bunches_then_stack(lambda i: same[i % ndist], N, H, W, np.uint16, out_dev=out.ptr, stacks=stacks, results_buf=results,
                                   info=info, zero_copy=not args.pageable, mosaic=cfa)
                return info["stage1_s"]
            run_packed()
            with_p, without = [], []
            for _ in range(3):
                with_p.append(run_packed())
                without.append(run_same())
            for s_ in stacks:
                s_.sync()
            if args.sitecorr:
                # the packed run once more with site corrections set on every stage-1 handle (black deltas and four 17 x 13
                # gain maps: what a phone's DNG carries), in turns with the packed run without them
                def _map(seed):
                    n = np.random.default_rng(seed).uniform(0.8, 1.6, size=(13, 17))
                    return dng.GainMap(n, spacing=(1.0 / 12, 1.0 / 16))
                # (deltas >= 0: the frames' black level is 0, so black + delta_h + delta_v has no room below)
                sc = dng.SiteCorrections(black_h=np.arange(W) % 3, black_v=np.arange(H) % 3, gains=[_map(k) for k in range(4)])

                def run_corrected():
                    for s_ in stacks:
                        s_.set_site_correction(sc)
                    try:
                        return run_packed()
                    finally:
                        for s_ in stacks:
                            s_.set_site_correction(None)
                run_corrected()
                with_s, plain_p = [], []
                for _ in range(3):
                    with_s.append(run_corrected())
                    plain_p.append(run_packed())
                for s_ in stacks:
                    s_.sync()
                developed.update({"sitecorr_packed_stage1_seconds": with_s, "packed_stage1_seconds_in_turns_sitecorr": plain_p,
                                  "sitecorr_over_packed_stage1": float(np.median(with_s) / np.median(plain_p))})
            if args.ljpeg:
                def run_ljpeg():
                    info = {}
                    bunches_then_stack(lambda i: lj[i % ndist], N, H, W, np.uint16, out_dev=out.ptr, stacks=stacks, results_buf=results,
                                       info=info, zero_copy=not args.pageable, packed=True)
                    return info["stage1_s"]
                run_ljpeg()
                with_l, with_p2, without2 = [], [], []
                for _ in range(3):
                    with_l.append(run_ljpeg())
                    with_p2.append(run_packed())
                    without2.append(run_same())
                for s_ in stacks:
                    s_.sync()
                    assert s_.ljpeg_status() == 0
                if args.split:
                    # the compressed run once more with the split path set on every stage-1 handle (decode inside a segment,
                    # kernels_ljpeg_split.hpp), in turns with the serial kernel on the same spans
                    def run_split():
                        for s_ in stacks:
                            s_.set_ljpeg_split(True)
                        try:
                            return run_ljpeg()
                        finally:
                            for s_ in stacks:
                                s_.set_ljpeg_split(False)
                    run_split()
                    with_sp, with_l2 = [], []
                    for _ in range(3):
                        with_sp.append(run_split())
                        with_l2.append(run_ljpeg())
                    for s_ in stacks:
                        s_.sync()
                        assert s_.ljpeg_status() == 0
                    developed.update({"ljpeg_split_stage1_seconds": with_sp, "ljpeg_stage1_seconds_in_turns_with_split": with_l2,
                                      "ljpeg_split_over_ljpeg_stage1": float(np.median(with_sp) / np.median(with_l2))})
                developed.update({"ljpeg_stage1_seconds": with_l, "packed_stage1_seconds_in_turns": with_p2,
                                  "mosaic_stage1_seconds_in_turns_with_ljpeg": without2,
                                  "ljpeg_over_packed_stage1": float(np.median(with_l) / np.median(with_p2)),
                                  "ljpeg_host_to_device_bytes": pushed * int(np.mean([f.span.nbytes for f in lj])),
                                  "ljpeg_bytes_over_mosaic_bytes": float(np.mean([f.span.nbytes for f in lj]) / (H * W * 2))})
            developed.update({"packed_bits": bits, "packed_stage1_seconds": with_p, "mosaic_stage1_seconds_in_turns": without,
                              "packed_over_mosaic_stage1": float(np.median(with_p) / np.median(without)),
                              "packed_host_to_device_bytes": pushed * int(pk[0].span.nbytes),
                              "packed_bytes_over_mosaic_bytes": pk[0].span.nbytes / (H * W * 2)})
        _, b1, _ = run()        # BGR stage 1 once more, after the mosaic runs: the two are compared inside one process
        extra = {"mosaic": {"stage1_seconds": m1, "stage2_seconds": m2, "bgr_stage1_seconds": s1, "bgr_stage1_seconds_again": b1,
                            "host_to_device_bytes": pushed * per // 3, "bgr_host_to_device_bytes": pushed * per,
                            "host_to_device_GB_per_s": pushed * per / 3 / m1 / 1e9, "upload_s": upload_s / 3, "compute_s": compute_s,
                            "stage1_Mpixels_per_s": pushed * H * W / m1 / 1e6, "speedup_over_bgr_stage1": s1 / m1, **developed}}
    print(json.dumps({"config": f"{N} x {W}x{H} u16 frames from {'pageable' if args.pageable else 'PINNED'} host memory -> "
                                f"{len(bunches)} bunches of <= 10 (overlap 2) -> one stack over the {len(bunches)} bunch results "
                                f"(resident, uint16), one GPU",
                      "frames_pushed_stage1": pushed, "stage1_seconds": s1, "stage2_seconds": s2, "seconds": s1 + s2,
                      "stage1_Mpixels_per_s": pushed * H * W / s1 / 1e6, "stage2_Mpixels_per_s": len(bunches) * H * W / s2 / 1e6,
                      "host_to_device_GB_per_s": pushed * per / s1 / 1e9,
                      "pinned_memcpy_GB_per_s": pinned_rate / 1e9, "upload_s": upload_s, "compute_s": compute_s, "wall_s": s1,
                      "overlap_efficiency": max(upload_s, compute_s) / s1,
                      "results_buffer_GB": per * nbunch / 1e9, "results_alloc_s": results_alloc_s,
                      "stage1_handles": nst - 1, "upload_path": "bounce copy (3 pinned buffers, copy-thread pool)" if args.pageable else
                                     "zero-copy from pinned frames (mi_stack_push_frame_pinned)", **extra}))
    for s_ in stacks:
        s_.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=5792)
    ap.add_argument("--width", type=int, default=8640)
    ap.add_argument("--two-stage", action="store_true",
                    help="the whole config-5 flow on this GPU: bunches from host memory, then the bunch results -- kept on "
                         "the device, truncated to uint16 as the reference's intermediate files are -- fused once more "
                         "(pipeline.bunches_then_stack)")
    ap.add_argument("--one-handle", action="store_true", help="stage 1 on a single handle (no overlap across bunches)")
    ap.add_argument("--mosaic", action="store_true", help="with --two-stage: stage 1 from the frames' raw mosaics as well")
    ap.add_argument("--develop", action="store_true",
                    help="with --two-stage --mosaic: stage 1 once more with raw development (colour matrix, sRGB curve, defect "
                         "sites) on the demosaic, beside the plain mosaic run")
    ap.add_argument("--calibrate", action="store_true",
                    help="with --two-stage --mosaic: stage 1 with a master dark and a flat field applied to every mosaic on the "
                         "device, in turns with the plain mosaic run")
    ap.add_argument("--sitecorr", action="store_true",
                    help="with --two-stage --mosaic --packed BITS: the packed stage 1 once more with site corrections (black deltas, "
                         "four gain maps) set on the handles, in turns with the packed run without them")
    ap.add_argument("--packed", type=int, default=0, choices=(0, 10, 12, 14, 16),
                    help="with --two-stage --mosaic: stage 1 from packed spans of that many bits (the file's bytes, unpacked on the "
                         "device), in turns with the mosaic run on the same samples")
    ap.add_argument("--ljpeg", action="store_true",
                    help="with --two-stage --mosaic --packed BITS: stage 1 from lossless-JPEG spans of the same samples as well")
    ap.add_argument("--split", action="store_true",
                    help="with --two-stage --mosaic --packed BITS --ljpeg: the compressed stage 1 once more through the split path "
                         "(Stack.set_ljpeg_split), in turns with the serial kernel")
    ap.add_argument("--pageable", action="store_true", help="host frames in ordinary (pageable) memory: the bounce-copy path")
    args = ap.parse_args()
    if args.two_stage:
        return two_stage(args)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dev = int(os.environ.get("MI_TOOL_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from shinestacker_amd import _lib as L
    from shinestacker_amd.actions import get_bunches, shard_steps
    N, H, W = args.frames, args.height, args.width
    per = H * W * 3 * 2
    ndist = 8   # distinct host frames, cycled
    buf = L.DeviceBuffer(per * ndist, dev)
    L.synth_frames_device(buf.ptr, np.uint16, H, W, 0, ndist, ndist, device=dev)
    host = [buf.download((H, W, 3), np.uint16, offset=i * per) for i in range(ndist)]
    all_bunches = get_bunches(list(range(N)), 10, 2)
    bunches = [all_bunches[i] for i in shard_steps(len(all_bunches), rank, world)]
    st = L.Stack(H, W, in_dtype=np.uint16, out_dtype=np.uint16, device=dev)
    out = L.DeviceBuffer(per, dev)

    def run():
        pushed = 0
        for b in bunches:
            st.reset()
            for f in b:
                st.push_frame(host[f % ndist], zero_copy=not args.pageable)
                pushed += 1
            st.finish_device(out.ptr)
        st.sync()
        return pushed
    run()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    pushed = run()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt, float(pushed)], dtype=torch.float64)
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        dt, pushed = float(tmax[0]), int(t[1])
        dist.barrier()
    if rank == 0:
        print(json.dumps({"config": f"{N} x {W}x{H} u16 frames from host memory, {len(all_bunches)} bunches of <= 10 "
                                    f"(overlap 2) over {world} process(es)",
                          "frames_pushed": pushed, "seconds": dt, "Mpixels_per_s": pushed * H * W / dt / 1e6,
                          "host_to_device_GB_per_s": pushed * per / dt / 1e9}))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
