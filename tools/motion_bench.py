#!/usr/bin/env python3
"""Motion export cost (k_motion, csrc/vp9hip_motion.hip) against a device-to-device copy, and
the cost of export on through the batch API.

kernel: one k_motion launch over `--frames` synthetic inter frames (the bench's synthetic
density: vp9hip_synth_frame's defaults, 4 tile columns at 4K) of 3840x2160 and of 1920x1080,
each repetition between two HIP events on the launch's stream, medians: us per launch, GB/s
over the bytes it has to move (52-byte blocks read + 12 bytes per cell written) and the ratio
to a hipMemcpyAsync device-to-device copy that moves the same total (it copies half of it:
every copied byte is read once and written once), timed the same way in the same run. Both
work-distribution shapes are timed: the flat-task kernel the runtime launches, and one thread
per block looping over its cells. Each shape's output is compared with vp9hip_motion_host.

batch: C2 and C3 as bench.py stages them (`--batch-frames` frames, one batch, replayed), export
off and on alternating, `--runs` runs each: ms per run_batch + sync, medians of `--steps`.

    python tools/motion_bench.py [--out profiles/NAME.json] [--sections kernel,batch]

Prints one JSON line. Needs a GPU; there is no fallback.
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library: they share libamdhip64 (see _torch_first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
v9 = importlib.import_module("ffmpeg-hybrid_amd")

MOTION_FRAME = np.dtype([("blk0", "<u4"), ("nblk", "<u4"), ("cols8", "<u4"), ("rows8", "<u4"), ("mv", "<u8"),
                         ("info", "<u8"), ("pitch", "<u4"), ("pad", "<u4")])   # MotionFrame (csrc/vp9hip_motion.h)


def timed(fn, warmup, reps):
    """Median / min / max ms of fn() between two events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def kernel_case(L, stream, w, h, log2, n, args):
    frames = [v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x6d6f7600 + i, inter=1, log2_tile_cols=log2)) for i in range(n)]
    cols8, rows8 = (w + 7) >> 3, (h + 7) >> 3
    gw, gh = 2 * cols8, 2 * rows8
    raw = b"".join(ctypes.string_at(f.pkt.blocks, f.pkt.nblocks * ctypes.sizeof(v9.Block)) for f in frames)
    blocks = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    mv = torch.empty((n, gh, gw, 2, 2), dtype=torch.int16, device="cuda")
    info = torch.empty((n, gh, gw, 4), dtype=torch.uint8, device="cuda")
    rec = np.zeros(n, MOTION_FRAME)
    blk0 = 0
    for i, f in enumerate(frames):
        rec[i] = (blk0, f.pkt.nblocks, cols8, rows8, mv[i].data_ptr(), info[i].data_ptr(), gw, 0)
        blk0 += f.pkt.nblocks
    recs = torch.frombuffer(bytearray(rec.tobytes()), dtype=torch.uint8).cuda()
    max_blk = max(f.pkt.nblocks for f in frames)
    read, written = len(raw), n * gw * gh * 12
    want = [v9.motion_host(f) for f in frames[:2]]
    out = {"size": [w, h], "frames": n, "blocks": blk0, "cells": n * gw * gh, "bytes_read": read, "bytes_written": written,
           "shapes": {}}
    for shape, name in ((0, "flat tasks (k_motion)"), (1, "one thread per block (k_motion_loop)")):
        def launch():
            if L.vp9hip_motion_launch_dev(recs.data_ptr(), n, max_blk, blocks.data_ptr(), shape, stream) != 0:
                raise RuntimeError("vp9hip_motion_launch_dev failed")
        mv.fill_(0x55)
        info.fill_(0x55)
        launch()
        torch.cuda.synchronize()
        for i, (wmv, winfo) in enumerate(want):
            if not (np.array_equal(mv[i].cpu().numpy(), wmv) and np.array_equal(info[i].cpu().numpy(), winfo)):
                raise RuntimeError("shape %d: frame %d differs from vp9hip_motion_host" % (shape, i))
        t = timed(launch, args.warmup, args.reps)
        out["shapes"][name] = {"ms": {"median": t[0], "min": t[1], "max": t[2]}, "GBps": (read + written) / t[0] / 1e6}
    half = (read + written) // 2
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    src.fill_(0x33)

    def copy():
        if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, 3, stream) != 0:    # hipMemcpyDeviceToDevice
            raise RuntimeError("hipMemcpyAsync failed")
    c = timed(copy, args.warmup, args.reps)
    out["copy_ms"] = {"median": c[0], "min": c[1], "max": c[2]}
    out["copy_GBps"] = (read + written) / c[0] / 1e6
    for s in out["shapes"].values():
        s["ratio_to_copy"] = c[0] / s["ms"]["median"]
    return out


def batch_case(config, args):
    sys.path.insert(0, ROOT)
    import bench
    frames, refs, (w, h, bpp, _, _) = bench.make_frames(v9, config, args.batch_frames)
    n = len(frames)
    res = {"config": config, "frames": n, "off_ms": [], "on_ms": []}
    for run in range(args.runs):
        for on in (0, 1):
            dev = v9.Device(0)
            if on:
                dev.set_export(motion=True)
            dev.configure(w, h, bpp, nbufs=n)
            dev.set_timing(False)
            dev.stage_batch(frames, list(range(n)), refs if any(r is not None for r in refs) else None)
            ms = []
            for step in range(args.batch_warmup + args.steps):
                t0 = time.perf_counter()
                dev.run_batch()
                dev.sync()
                if step >= args.batch_warmup:
                    ms.append(1e3 * (time.perf_counter() - t0))
            if on and run == 0:
                got, want = dev.download_motion(n - 1), v9.motion_host(frames[n - 1])
                if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                    raise RuntimeError("%s: the exported field differs from vp9hip_motion_host" % config)
            dev.close()
            res["on_ms" if on else "off_ms"].append(statistics.median(ms))
    off, on = statistics.median(res["off_ms"]), statistics.median(res["on_ms"])
    res.update(off_fps=1e3 * n / off, on_fps=1e3 * n / on, on_minus_off_ms=on - off, on_over_off=on / off)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sections", default="kernel,batch", help="comma list of kernel, batch")
    ap.add_argument("--batch-frames", type=int, default=32)
    ap.add_argument("--batch-warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sections = set(args.sections.split(","))
    L = v9.lib()
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    res = {"tool": "motion_bench", "device": v9.device_info(0)[1], "reps": args.reps}
    if "kernel" in sections:
        side = torch.cuda.Stream()                             # a stream of torch's own: launches go to it directly
        torch.cuda.set_stream(side)
        stream = side.cuda_stream
        assert stream, "the timed stream must not be the null stream"
        res["kernel"] = [kernel_case(L, stream, 3840, 2160, 2, args.frames, args),
                         kernel_case(L, stream, 1920, 1080, 0, args.frames, args)]
    if "batch" in sections:
        res["batch"] = [batch_case(c, args) for c in ("C2", "C3")]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
