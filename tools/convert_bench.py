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

The resample cases (vp9hip_convert_frames_resampled: triangle filter, source rectangles) are
timed the same way: the triangle to rgbp_f16 beside the full-size conversion followed by
torch.nn.functional.interpolate(mode="bilinear", antialias=True) of the half tensor (what a
caller does without it), beside the box kernel (resize= alone) and the new kernel's own box
filter at the same shapes; 32 rectangles of 256x256 out of 4 frames to 224x224; a 1920x1080 ->
3840x2160 triangle upscale to rgb24; each with the copy of the same total bytes.

The bicubic cases (vp9hip_convert_frames_bicubic) are `--frames` frames to 224x224 rgbp_f16, the
whole output and letterboxed (letterbox_rect), each timed beside the triangle kernel on the same
inputs and beside the full-size conversion followed by
torch.nn.functional.interpolate(mode="bicubic", antialias=True) of the half tensor to the
picture's size (the letterbox's paste into the fill is left out of that yardstick, in its favour).

    python tools/convert_bench.py [--out profiles/NAME.json] [--sections convert,resize,resample,bicubic]

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


def resample_cases(dev, args, copy_of, w, h, n):
    """The cases of the fused resampling; copy_of(bytes) times the copy of that total."""
    out_cases = []

    def entry(name, bpp, fmt, src_wh, frames, ow, oh, read, fn, **more):
        written = frames * v9.out_layout(fmt, ow, oh, bpp)[0]
        t = timed(fn, args.warmup, args.reps)
        cpy = copy_of(read + written)
        e = {"case": name, "bpp": bpp, "format": fmt, "source": list(src_wh), "frames": frames, "resize": [ow, oh],
             "bytes_read": read, "bytes_written": written, "ms": {"median": t[0], "min": t[1], "max": t[2]},
             "copy_ms": {"median": cpy[0], "min": cpy[1], "max": cpy[2]}, "ratio_to_copy": cpy[0] / t[0]}
        e.update(more)
        out_cases.append(e)
        return t[0]

    bufs = list(range(n))
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    read = n * (w * h + 2 * cw * ch)
    dev.configure(w, h, 8, nbufs=n)
    dev.fill(0, n, 0x55)
    dev.sync()
    fmt = "rgbp_f16"
    for ow, oh in ((224, 224), (1920, 1080)):
        out = torch.empty(n * v9.out_layout(fmt, ow, oh, 8)[0], dtype=torch.uint8, device="cuda")
        what = "%dx%d" % (ow, oh)
        t_old = entry("box, k_convert_scale " + what, 8, fmt, (w, h), n, ow, oh, read,
                      lambda: dev.convert(bufs, fmt, colorspace=2, out=out, resize=(ow, oh)))
        t_box = entry("box, k_convert_resample " + what, 8, fmt, (w, h), n, ow, oh, read,
                      lambda: dev.convert(bufs, fmt, colorspace=2, out=out, resize=(ow, oh), src_rects=(0, 0, w, h)))
        more = {}
        if (ow, oh) == (224, 224):     # the bar: the full-size conversion, then the framework's antialiased bilinear
            full = torch.empty(n * v9.out_layout(fmt, w, h, 8)[0], dtype=torch.uint8, device="cuda")

            def two_step():
                r = dev.convert(bufs, fmt, colorspace=2, out=full)
                return torch.nn.functional.interpolate(r, size=(oh, ow), mode="bilinear", antialias=True)
            try:
                two = timed(two_step, max(2, args.warmup // 4), max(5, args.reps // 4))
                more["convert_then_framework_resize_ms"] = {"median": two[0], "min": two[1], "max": two[2]}
            except RuntimeError as e:      # reported, not worked around: the yardstick is what it is
                two = None
                more["convert_then_framework_resize_error"] = str(e)[:300]
            del full
        t_tri = entry("triangle " + what, 8, fmt, (w, h), n, ow, oh, read,
                      lambda: dev.convert(bufs, fmt, colorspace=2, out=out, resize=(ow, oh), filter="triangle"), **more)
        out_cases[-1]["ratio_to_box_kernel"] = t_tri / t_old
        out_cases[-2]["ratio_to_box_kernel"] = t_box / t_old
        if more.get("convert_then_framework_resize_ms"):
            out_cases[-1]["speedup_over_two_steps"] = more["convert_then_framework_resize_ms"]["median"] / t_tri
        del out
    # 32 rectangles of 256 x 256 out of 4 frames
    rects = [(256 * (3 + i % 8), 256 * (1 + i // 8), 256, 256) for i in range(32)]
    out = torch.empty(32 * v9.out_layout(fmt, 224, 224, 8)[0], dtype=torch.uint8, device="cuda")
    order = [i % 4 for i in range(32)]
    entry("triangle, 32 rectangles of 256x256 from 4 frames", 8, fmt, (w, h), 32, 224, 224, 32 * 256 * 256 * 3 // 2,
          lambda: dev.convert(order, fmt, colorspace=2, out=out, resize=(224, 224), filter="triangle", src_rects=rects))
    # the same launch with its arguments built once: Device.convert builds 32 rectangles per call,
    # and the interval between the two events contains the host's part of the call
    desc = v9.OutDesc(v9.OUT_FORMATS[fmt], 2, 0, w, h, 0, 0)
    rect_arr = (v9.Rect * 32)(*[v9.Rect(*r) for r in rects])
    rs = v9.Resample(v9.FILTERS["triangle"], 224, 224, ctypes.cast(rect_arr, ctypes.POINTER(v9.Rect)))
    arr = (ctypes.c_int * 32)(*order)
    st, ptr = torch.cuda.current_stream().cuda_stream, out.data_ptr()

    def direct():
        if v9.lib().vp9hip_convert_frames_resampled(dev._c, arr, 32, ctypes.byref(desc), ctypes.byref(rs), ptr, st) != 0:
            raise RuntimeError("vp9hip_convert_frames_resampled failed")
    entry("triangle, 32 rectangles of 256x256 from 4 frames, arguments built once", 8, fmt, (w, h), 32, 224, 224,
          32 * 256 * 256 * 3 // 2, direct)
    del out
    # upscale
    sw, sh = 1920, 1080
    dev.configure(sw, sh, 8, nbufs=n)
    dev.fill(0, n, 0x55)
    dev.sync()
    out = torch.empty(n * v9.out_layout("rgb24", 3840, 2160, 8)[0], dtype=torch.uint8, device="cuda")
    entry("triangle upscale", 8, "rgb24", (sw, sh), n, 3840, 2160, n * sw * sh * 3 // 2,
          lambda: dev.convert(bufs, "rgb24", colorspace=2, out=out, resize=(3840, 2160), filter="triangle"))
    del out
    return out_cases


def bicubic_cases(dev, args, w, h, n):
    """The bicubic kernel, the triangle kernel and the two-step path on the same inputs."""
    cases = []
    bufs = list(range(n))
    fmt, ow, oh = "rgbp_f16", 224, 224
    dev.configure(w, h, 8, nbufs=n)
    dev.fill(0, n, 0x55)
    dev.sync()
    out = torch.empty(n * v9.out_layout(fmt, ow, oh, 8)[0], dtype=torch.uint8, device="cuda")
    full = torch.empty(n * v9.out_layout(fmt, w, h, 8)[0], dtype=torch.uint8, device="cuda")
    for name, dst in (("whole output", None), ("letterbox", v9.letterbox_rect(w, h, ow, oh))):
        pw, ph = (ow, oh) if dst is None else dst[2:]
        cub = timed(lambda: dev.convert(bufs, fmt, colorspace=2, out=out, resize=(ow, oh), filter="bicubic", dst_rects=dst),
                    args.warmup, args.reps)
        tri = timed(lambda: dev.convert(bufs, fmt, colorspace=2, out=out, resize=(ow, oh), filter="triangle", dst_rects=dst),
                    args.warmup, args.reps)

        def two_step():
            r = dev.convert(bufs, fmt, colorspace=2, out=full)
            return torch.nn.functional.interpolate(r, size=(ph, pw), mode="bicubic", antialias=True)
        e = {"case": name, "bpp": 8, "format": fmt, "source": [w, h], "frames": n, "resize": [ow, oh],
             "dst_rect": None if dst is None else list(dst),
             "bicubic_ms": {"median": cub[0], "min": cub[1], "max": cub[2]},
             "triangle_ms": {"median": tri[0], "min": tri[1], "max": tri[2]},
             "ratio_to_triangle": cub[0] / tri[0], "us_per_frame": 1e3 * cub[0] / n}
        try:
            two = timed(two_step, max(2, args.warmup // 4), max(5, args.reps // 4))
            e["convert_then_framework_resize_ms"] = {"median": two[0], "min": two[1], "max": two[2]}
            e["speedup_over_two_steps"] = two[0] / cub[0]
        except RuntimeError as err:      # reported, not worked around: the yardstick is what it is
            e["convert_then_framework_resize_error"] = str(err)[:300]
        cases.append(e)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", default=None,
                    help="comma list of cases to run, e.g. rgb24,rgbp_f16@224x224 (default: all); for profiler runs")
    ap.add_argument("--sections", default="convert,resize,resample,bicubic",
                    help="comma list of convert, resize, resample, bicubic")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sections = set(args.sections.split(","))
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
        if "convert" not in sections or (only is not None and fmt not in only):
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
        if "resize" not in sections or (only is not None and "%s@%dx%d" % (fmt, ow, oh) not in only):
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
    if "resample" in sections and only is None:
        def copy_of(total):
            half = total // 2
            src = torch.empty(half, dtype=torch.uint8, device="cuda")
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            src.fill_(0x33)

            def copy():
                if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, D2D, stream) != 0:
                    raise RuntimeError("hipMemcpyAsync failed")
            return timed(copy, args.warmup, args.reps)
        res["resample_cases"] = resample_cases(dev, args, copy_of, w, h, n)
    if "bicubic" in sections and only is None:
        res["bicubic_cases"] = bicubic_cases(dev, args, w, h, n)
    dev.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
