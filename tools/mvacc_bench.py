#!/usr/bin/env python3
"""Accumulated motion cost (k_mvacc, csrc/vp9hip_mvacc.hip) against a device-to-device copy, and
the cost of the flag through the batch API.

kernel: `--frames` synthetic inter frames (vp9hip_synth_frame's defaults, 4 tile columns at 4K)
of 3840x2160 and of 1920x1080, their mv / info planes resident (vp9hip_motion_host's output), in
chains of depth 1, 4 and 16 inside one batch: frame i follows frame i - 1 under every reference
name unless i is a multiple of the depth, when its parent is a finished record plane outside the
batch. Each repetition runs between two HIP events on the launches' stream, medians: us, and the
ratio to a hipMemcpyAsync device-to-device copy of cells x (12 read + 16 written) bytes in total
(it copies half of it: every copied byte is read once and written once), timed the same way in
the same run. Both kernel shapes are timed: one launch per chain position, each reading only
finished records, which the runtime launches, and the walk (one launch, every lane follows its
chain through the batch's mv / info planes). Each shape's output is compared with vp9hip_motion_acc_host first.

batch: C2 and C3 as bench.py stages them (`--batch-frames` frames, one batch, replayed): no
export, the motion export, and the motion export with accumulated motion, alternating, `--runs`
runs each: ms per run_batch + sync, medians of `--steps`.

    python tools/mvacc_bench.py [--out profiles/NAME.json] [--sections kernel,batch]

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

# AccFrame (csrc/vp9hip_mvacc.h)
ACC_FRAME = np.dtype([("mv", "<u8"), ("info", "<u8"), ("acc", "<u8"), ("gw", "<u4"), ("gh", "<u4"), ("pitch", "<u4"),
                      ("serial", "<u4"), ("par", "<i4", 3), ("level", "<u4"), ("ext", "<u8", 3)])
PAR_EXT = -1


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


def kernel_cases(L, stream, w, h, log2, n, args):
    frames = [v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x6d766100 + i, inter=1, log2_tile_cols=log2)) for i in range(n)]
    fields = [v9.motion_host(f) for f in frames]
    del frames
    gh, gw = fields[0][1].shape[:2]
    cells = n * gw * gh
    mv = torch.from_numpy(np.stack([f[0] for f in fields])).cuda()
    info = torch.from_numpy(np.stack([f[1] for f in fields])).cuda()
    acc = torch.empty((n, gh, gw, 4), dtype=torch.int32, device="cuda")
    ext_h = np.zeros((gh, gw), v9.ACC_CELL)                     # the finished records outside the batch
    ext_h["dx"], ext_h["root"], ext_h["hops"] = np.arange(gw)[None, :], 9, 3
    ext = torch.from_numpy(ext_h.view("<i4").reshape(gh, gw, 4).copy()).cuda()
    half = cells * 28 // 2
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    src.fill_(0x33)

    def copy():
        if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, 3, stream) != 0:    # hipMemcpyDeviceToDevice
            raise RuntimeError("hipMemcpyAsync failed")
    out = []
    for depth in args.depths:
        rec = np.zeros(n, ACC_FRAME)
        want = []
        for i in range(n):
            head = i % depth == 0
            rec[i] = (mv[i].data_ptr(), info[i].data_ptr(), acc[i].data_ptr(), gw, gh, gw, 100 + i,
                      (PAR_EXT if head else i - 1,) * 3, i % depth, (ext.data_ptr() if head else 0,) * 3)
            want.append(v9.motion_acc_host(fields[i][0], fields[i][1], 100 + i, [ext_h if head else want[i - 1]] * 3))
        recs = torch.frombuffer(bytearray(rec.tobytes()), dtype=torch.uint8).cuda()
        order_h = np.array(sorted(range(n), key=lambda i: (i % depth, i)), np.uint32)
        order = torch.from_numpy(order_h.view(np.int32)).cuda()
        level_n = (ctypes.c_int * depth)(*[sum(1 for i in range(n) if i % depth == l) for l in range(depth)])
        res = {"size": [w, h], "frames": n, "depth": depth, "cells": cells, "bytes": cells * 28, "shapes": {}}
        for shape, name in ((0, "one launch per chain position (k_mvacc)"), (1, "walk, one launch")):
            def launch():
                if L.vp9hip_mvacc_launch_dev(recs.data_ptr(), n, gw, gh, shape, order.data_ptr(), level_n, depth, stream) != 0:
                    raise RuntimeError("vp9hip_mvacc_launch_dev failed")
            acc.fill_(0x55555555)
            launch()
            torch.cuda.synchronize()
            got = acc.cpu().numpy()
            for i in range(n):
                if got[i].tobytes() != want[i].tobytes():
                    raise RuntimeError("%dx%d depth %d shape %d: frame %d differs from vp9hip_motion_acc_host" % (w, h, depth, shape, i))
            t = timed(launch, args.warmup, args.reps)
            res["shapes"][name] = {"us": {"median": 1e3 * t[0], "min": 1e3 * t[1], "max": 1e3 * t[2]}}
        c = timed(copy, args.warmup, args.reps)
        res["copy_us"] = {"median": 1e3 * c[0], "min": 1e3 * c[1], "max": 1e3 * c[2]}
        for s in res["shapes"].values():
            s["ratio_to_copy"] = s["us"]["median"] / res["copy_us"]["median"]
        out.append(res)
    return out


def batch_case(config, args):
    import bench
    frames, refs, (w, h, bpp, _, _) = bench.make_frames(v9, config, args.batch_frames)
    n = len(frames)
    modes = ("off", "motion", "motion_acc")
    res = {"config": config, "frames": n, "ms": {m: [] for m in modes}}
    for run in range(args.runs):
        for m in modes:
            dev = v9.Device(0)
            if m != "off":
                dev.set_export(motion=True, motion_acc=m == "motion_acc")
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
            if m == "motion_acc" and run == 0:
                res["max_hops"] = int(dev.download_motion_acc(n - 1)[0]["hops"].max())
            dev.close()
            res["ms"][m].append(statistics.median(ms))
    med = {m: statistics.median(res["ms"][m]) for m in modes}
    res.update(median_ms=med, fps={m: 1e3 * n / med[m] for m in modes},
               acc_minus_motion_ms=med["motion_acc"] - med["motion"], acc_over_motion=med["motion_acc"] / med["motion"],
               acc_over_off=med["motion_acc"] / med["off"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--depths", type=lambda s: [int(x) for x in s.split(",")], default=[1, 4, 16])
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
    res = {"tool": "mvacc_bench", "device": v9.device_info(0)[1], "reps": args.reps}
    if "kernel" in sections:
        side = torch.cuda.Stream()                             # a stream of torch's own: launches go to it directly
        torch.cuda.set_stream(side)
        stream = side.cuda_stream
        assert stream, "the timed stream must not be the null stream"
        res["kernel"] = kernel_cases(L, stream, 3840, 2160, 2, args.frames, args) + \
            kernel_cases(L, stream, 1920, 1080, 0, args.frames, args)
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
