#!/usr/bin/env python3
"""Residual export cost (k_residual, csrc/vp9hip_residual.hip) against two yardsticks, and the
cost of export on through the batch API.

kernel: `--frames` synthetic 3840x2160 8-bit keyframes (4 tile columns) and `--frames` 1920x1080
inter frames (behind the keyframe they predict from) at the generator's default density, each
staged as one batch and run once, so the planner's records are resident. The exported planes are
first compared with vp9hip_residual_host.
Then the export (one k_residual launch over the batch: it writes the zeros itself, there is no
separate clear) is repeated between two HIP events on a stream of the tool's own, medians of
`--reps` after `--warmup`, and in the same run, timed the same way:
  (a) a hipMemcpyAsync device-to-device copy that moves the same bytes (coefficients read + coded
      planes written; it copies half of the total: every copied byte is read once and written once);
  (b) the summed time of the batch's own residual launches (k_resid of Device.timing(), a run with
      per-launch events): the same transforms over the same coefficients, without the placement.
      Keyframe batches run part of their residuals inside the fused intra launches (k_plf), whose
      time is reported beside it and not added.

batch: C2 and C3 as bench.py stages them (`--batch-frames` frames, one batch, replayed), export
off and on alternating, `--runs` runs each: ms per run_batch + sync, medians of `--steps`.

    python tools/residual_bench.py [--out profiles/NAME.json] [--sections kernel,batch]

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
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def kernel_case(L, stream, w, h, log2, inter, n, args):
    if inter:
        frames = [v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x72657300 + i, inter=int(i > 0), log2_tile_cols=log2))
                  for i in range(n + 1)]
        refs = [None] + [(i - 1,) * 3 for i in range(1, n + 1)]
    else:
        frames = [v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x72657300 + i, log2_tile_cols=log2)) for i in range(n)]
        refs = None
    dev = v9.Device(0)
    dev.set_export(motion=False, residual=True)
    dev.configure(w, h, 8, nbufs=len(frames))
    dev.stage_batch(frames, list(range(len(frames))), refs)
    dev.set_timing(True)                                       # per-launch events: yardstick (b)
    dev.run_batch()
    dev.sync()
    tm = dev.timing()
    dev.set_timing(False)
    dev.run_batch()
    dev.sync()
    for i in (len(frames) - 1, len(frames) - 2):
        got, want = dev.download_residual(i), v9.residual_host(frames[i])
        if not all(np.array_equal(g, x) for g, x in zip(got, want)):
            raise RuntimeError("%dx%d frame %d differs from vp9hip_residual_host" % (w, h, i))
    # the launch covers every frame of the batch (the inter workload's leading keyframe included)
    read = sum(f.pkt.ncoefs * 2 for f in frames)
    written = len(frames) * sum(r * c * 2 for r, c in v9.residual_shapes(w, h))
    planes_bytes = len(frames) * (((w + 63) & ~63) * ((h + 63) & ~63) * 3)   # int16 planes of the padded 4:2:0 geometry

    def export():
        if L.vp9hip_residual_relaunch(dev._c, stream) != 0:
            raise RuntimeError("vp9hip_residual_relaunch failed")
    t = timed(export, args.warmup, args.reps)
    half = (read + written) // 2
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    src.fill_(0x33)

    def copy():
        if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, 3, stream) != 0:    # hipMemcpyDeviceToDevice
            raise RuntimeError("hipMemcpyAsync failed")
    c = timed(copy, args.warmup, args.reps)
    out = {"size": [w, h], "kind": "inter" if inter else "key", "frames": len(frames),
           "coefs": int(sum(f.pkt.ncoefs for f in frames)), "tx_blocks": int(sum(f.pkt.neobs for f in frames)),
           "bytes_read": int(read), "bytes_written": int(written), "plane_bytes_allocated": int(planes_bytes),
           "export_ms": t, "export_GBps": (read + written) / t["median"] / 1e6,
           "copy_ms": c, "copy_GBps": (read + written) / c["median"] / 1e6, "export_over_copy": t["median"] / c["median"],
           "timing_ms": {k: [ms, cnt] for k, (ms, cnt) in tm.items()},
           "k_resid_ms": tm["k_resid"][0], "export_over_k_resid": t["median"] / tm["k_resid"][0] if tm["k_resid"][0] else None}
    dev.close()
    return out


def batch_case(config, args):
    import bench
    frames, refs, (w, h, bpp, _, _) = bench.make_frames(v9, config, args.batch_frames)
    n = len(frames)
    res = {"config": config, "frames": n, "off_ms": [], "on_ms": []}
    for run in range(args.runs):
        for on in (0, 1):
            dev = v9.Device(0)
            if on:
                dev.set_export(motion=False, residual=True)
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
                got, want = dev.download_residual(n - 1), v9.residual_host(frames[n - 1])
                if not all(np.array_equal(g, x) for g, x in zip(got, want)):
                    raise RuntimeError("%s: the exported field differs from vp9hip_residual_host" % config)
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
    res = {"tool": "residual_bench", "device": v9.device_info(0)[1], "reps": args.reps}
    if "kernel" in sections:
        side = torch.cuda.Stream()                             # a stream of torch's own: launches go to it directly
        torch.cuda.set_stream(side)
        stream = side.cuda_stream
        assert stream, "the timed stream must not be the null stream"
        res["kernel"] = [kernel_case(L, stream, 3840, 2160, 2, 0, args.frames, args),
                         kernel_case(L, stream, 1920, 1080, 0, 1, args.frames, args)]
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
