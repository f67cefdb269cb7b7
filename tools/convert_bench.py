#!/usr/bin/env python3
"""Output conversion throughput (vp9hip_convert_frames, vp9hip_convert_frames_scaled) against a
device-to-device copy.

Times one launch over `--frames` frames of `--size` per case, each repetition between two
HIP events on the launch's stream, and reports the median: us per frame, GB/s over the bytes
the conversion has to move (visible source samples read + output bytes written), and the
ratio to a hipMemcpyAsync device-to-device copy that moves the same total (it copies half of
it: every copied byte is read once and written once), timed the same way in the same run.

The resize cases (the fused box-filter resize, Device.convert(resize=...)) are timed the same
way beside two yardsticks of the same run: (a) the copy of the same total bytes (visible source
read + the small output written), and (b) what a caller did without the fused kernel, on the
same stream: the full-size conversion followed by torch.nn.functional.interpolate(mode="area")
of the half tensor, or, for semi-planar, an adaptive average pool of the Y plane and of the UV
plane (as float: the framework pools no integer tensor).

    python tools/convert_bench.py [--out profiles/NAME.json]

Prints one JSON line. Needs a GPU; there is no fallback.
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import torch  # before the library: they share libamdhip64 (see _torch_first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
v9 = importlib.import_module("ffmpeg-hybrid_amd")

CASES = [(8, "rgb24"), (8, "rgbp_f16"), (10, "semiplanar")]
RESIZE_CASES = [(8, "rgbp_f16", (224, 224)), (8, "rgbp_f16", (1920, 1080)), (10, "semiplanar", (1920, 1080))]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", default=None,
                    help="comma list of cases to run, e.g. rgb24,rgbp_f16@224x224 (default: all); for profiler runs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w, h = (int(x) for x in args.size.split("x"))
    only = set(args.only.split(",")) if args.only else None
    n = args.frames
    L = v9.lib()
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    D2D = 3                                                     # hipMemcpyDeviceToDevice
    side = torch.cuda.Stream()                                 # a stream of torch's own: launches go to it directly
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream, "the timed stream must not be the null stream"
    dev = v9.Device(0)
    res = {"tool": "convert_bench", "size": [w, h], "frames": n, "reps": args.reps, "device": v9.device_info(0)[1],
           "cases": []}
    for bpp, fmt in CASES:
        if only is not None and fmt not in only:
            continue
        dev.configure(w, h, bpp, nbufs=n)
        dev.fill(0, n, 0x55)
        dev.sync()
        bs = 1 if bpp == 8 else 2
        cw, ch = (w + 1) >> 1, (h + 1) >> 1
        read = n * (w * h + 2 * cw * ch) * bs
        nbytes, _, _ = v9.out_layout(fmt, w, h, bpp)
        written = n * nbytes
        out = torch.empty(written, dtype=torch.uint8, device="cuda")
        bufs = list(range(n))
        cvt = timed(lambda: dev.convert(bufs, fmt, colorspace=2, out=out), args.warmup, args.reps)
        half = (read + written) // 2
        src = torch.empty(half, dtype=torch.uint8, device="cuda")
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        src.fill_(0x33)

        def copy():
            if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, D2D, stream) != 0:
                raise RuntimeError("hipMemcpyAsync failed")
        cpy = timed(copy, args.warmup, args.reps)
        total = read + written
        res["cases"].append({
            "bpp": bpp, "format": fmt, "bytes_read": read, "bytes_written": written,
            "convert_ms": {"median": cvt[0], "min": cvt[1], "max": cvt[2]},
            "copy_ms": {"median": cpy[0], "min": cpy[1], "max": cpy[2]},
            "us_per_frame": 1e3 * cvt[0] / n,
            "convert_GBps": total / cvt[0] / 1e6,
            "copy_GBps": total / cpy[0] / 1e6,
            "ratio_to_copy": cpy[0] / cvt[0],
        })
        del out, src, dst
    res["resize_cases"] = []
    for bpp, fmt, (ow, oh) in RESIZE_CASES:
        if only is not None and "%s@%dx%d" % (fmt, ow, oh) not in only:
            continue
        dev.configure(w, h, bpp, nbufs=n)
        dev.fill(0, n, 0x55)
        dev.sync()
        bs = 1 if bpp == 8 else 2
        cw, ch = (w + 1) >> 1, (h + 1) >> 1
        read = n * (w * h + 2 * cw * ch) * bs
        written = n * v9.out_layout(fmt, ow, oh, bpp)[0]
        out = torch.empty(written, dtype=torch.uint8, device="cuda")
        full = torch.empty(n * v9.out_layout(fmt, w, h, bpp)[0], dtype=torch.uint8, device="cuda")
        bufs = list(range(n))
        fused = timed(lambda: dev.convert(bufs, fmt, colorspace=2, out=out, resize=(ow, oh)), args.warmup, args.reps)

        def two_step():
            r = dev.convert(bufs, fmt, colorspace=2, out=full)
            if fmt == "semiplanar":
                y, uv = r
                och, ocw = (oh + 1) >> 1, (ow + 1) >> 1
                return (torch.nn.functional.adaptive_avg_pool2d(y.float(), (oh, ow)),
                        torch.nn.functional.adaptive_avg_pool2d(uv.permute(0, 3, 1, 2).float(), (och, ocw)))
            return torch.nn.functional.interpolate(r, size=(oh, ow), mode="area")
        two = timed(two_step, max(2, args.warmup // 4), max(5, args.reps // 4))
        half = (read + written) // 2
        src = torch.empty(half, dtype=torch.uint8, device="cuda")
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        src.fill_(0x33)

        def copy():
            if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, D2D, stream) != 0:
                raise RuntimeError("hipMemcpyAsync failed")
        cpy = timed(copy, args.warmup, args.reps)
        total = read + written
        res["resize_cases"].append({
            "bpp": bpp, "format": fmt, "resize": [ow, oh], "bytes_read": read, "bytes_written": written,
            "fused_ms": {"median": fused[0], "min": fused[1], "max": fused[2]},
            "copy_ms": {"median": cpy[0], "min": cpy[1], "max": cpy[2]},
            "convert_then_framework_resize_ms": {"median": two[0], "min": two[1], "max": two[2]},
            "us_per_frame": 1e3 * fused[0] / n,
            "fused_GBps": total / fused[0] / 1e6,
            "copy_GBps": total / cpy[0] / 1e6,
            "ratio_to_copy": cpy[0] / fused[0],
            "speedup_over_two_steps": two[0] / fused[0],
        })
        del out, full, src, dst
    dev.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
