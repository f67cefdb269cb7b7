#!/usr/bin/env python3
"""Residual tensors at model size (k_residual_scale, csrc/vp9hip_residual_scale.hip) against
three yardsticks timed in the same run, in one process, on a side stream of torch's.

Cases: `--frames` residual fields of 3840x2160 and of 1920x1080, 4:2:0 in a 10-bit context, to
224x224, as "rgb_f16" and as "yuv_i16". A field is the field of a decoded synthetic keyframe
overwritten with random codes in [-m, m] through Device.residual's views (two distinct fields,
alternating over the buffers). The outputs of every frame are first compared with
vp9hip_residual_scaled_host. Each repetition is timed between two HIP events on the launch's
stream; medians with min / max.

  (a) copy: a hipMemcpyAsync device-to-device copy of the bytes the launch reads plus those it
      writes.
  (b) framework: the same fields through Device.residual's views: widen to float, upsample
      chroma to luma size, the float matrix, interpolate(mode="area"), half.
  (c) k_convert_scale: the pixel conversion's fused resize ("rgbp_f16", same output size) over
      the pixel planes of the same buffers, a 10-bit source of the same size: the same bytes read
      through the same access shape.

Reported: the launch in us and GB/s over the bytes read, and the ratios to (a), (b) and (c)
(above 1: the launch is faster).

    python tools/residual_scale_bench.py [--out profiles/NAME.json]

Prints one JSON line. Needs a GPU; there is no fallback.
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch  # before the library: they share libamdhip64 (see _torch_first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
v9 = importlib.import_module("ffmpeg-hybrid_amd")

BPP = 10
KR, KB = .2126, .0722           # BT.709, limited range: the float matrix of the framework route


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


def case(L, stream, w, h, n, ow, oh, args):
    rng = np.random.default_rng(w)
    m = (1 << BPP) - 1
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    dev = v9.Device(0)
    dev.set_export(motion=False, residual=True)
    dev.configure(w, h, BPP, nbufs=n)
    dev.set_timing(False)
    key = v9.SynthFrame(v9.synth_params(w, h, BPP, seed=0x15c00))
    for b in range(n):
        dev.submit(key, b)
    dev.sync()
    host = [[rng.integers(-m, m + 1, s).astype(np.int16) for s in ((h, w), (ch, cw), (ch, cw))] for _ in range(2)]
    for b in range(n):
        for view, a in zip(dev.residual(b), host[b % 2]):
            view.copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    read = n * (w * h + 2 * cw * ch) * 2
    written = n * 3 * ow * oh * 2
    res = {"size": [w, h], "out": [ow, oh], "bpp": BPP, "frames": n, "bytes_read": read, "bytes_written": written}
    arr = (ctypes.c_int * n)(*range(n))
    out = torch.empty(n * 3 * oh * ow, dtype=torch.int16, device="cuda")
    for fmt in ("rgb_f16", "yuv_i16"):
        d = v9.ResidDesc(v9.RESID_FORMATS[fmt], 2, 0, ow, oh, 0, 0)

        def launch():
            if L.vp9hip_residual_frames_scaled(dev._c, arr, n, ctypes.byref(d), out.data_ptr(), stream) != 0:
                raise RuntimeError("vp9hip_residual_frames_scaled failed")
        # correctness first: every frame against the host statement of the definition
        want = [v9.residual_scaled_host(f, w, h, 1, 1, BPP, fmt, (ow, oh)).view(np.int16) for f in host]
        out.fill_(0x55)
        launch()
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(n, 3, oh, ow)
        for i in range(n):
            if not np.array_equal(got[i], want[i % 2]):
                raise RuntimeError("%dx%d %s: frame %d differs from vp9hip_residual_scaled_host" % (w, h, fmt, i))
        t = timed(launch, args.warmup, args.reps)
        res[fmt] = {"ms": t, "us": 1e3 * t["median"], "GBps": read / t["median"] / 1e6}
    # (a) a device-to-device copy of the bytes the launch reads plus those it writes
    src = torch.empty(read + written, dtype=torch.uint8, device="cuda")
    dst = torch.empty(read + written, dtype=torch.uint8, device="cuda")
    src.fill_(0x33)

    def copy():
        if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), read + written, 3, stream) != 0:    # hipMemcpyDeviceToDevice
            raise RuntimeError("hipMemcpyAsync failed")
    c = timed(copy, args.warmup, args.reps)
    res["copy"] = {"ms": c, "GBps": (read + written) / c["median"] / 1e6}
    del src, dst
    # (c) k_convert_scale over the pixel planes of the same buffers
    od = v9.OutDesc(v9.OUT_FORMATS["rgbp_f16"], 2, 0, w, h, 0, 0)

    def convert():
        if L.vp9hip_convert_frames_scaled(dev._c, arr, n, ctypes.byref(od), ow, oh, out.data_ptr(), stream) != 0:
            raise RuntimeError("vp9hip_convert_frames_scaled failed")
    k = timed(convert, args.warmup, args.reps)
    res["convert_scale"] = {"ms": k, "us": 1e3 * k["median"], "GBps": read / k["median"] / 1e6}
    # (b) the framework route on the same fields
    views = [dev.residual(b) for b in range(n)]
    sy, sc = m / (219. * (1 << (BPP - 8))), m / (224. * (1 << (BPP - 8)))
    kg = 1. - KR - KB
    mat = torch.tensor([[sy, 0., 2. * (1. - KR) * sc], [sy, -2. * KB * (1. - KB) / kg * sc, -2. * KR * (1. - KR) / kg * sc],
                        [sy, 2. * (1. - KB) * sc, 0.]], dtype=torch.float32, device="cuda") / m

    def framework():
        frames = []
        for y, u, v in views:
            uv = torch.stack([u, v]).float()[None]
            uv = torch.nn.functional.interpolate(uv, scale_factor=2, mode="nearest")[0, :, :h, :w]
            yuv = torch.cat([y.float()[None], uv])
            frames.append(torch.einsum("rc,chw->rhw", mat, yuv))
        return torch.nn.functional.interpolate(torch.stack(frames), size=(oh, ow), mode="area").half()
    ref = framework()
    torch.cuda.synchronize()
    # the float route is not the integer definition (it has no defined rounding): how far apart they are is reported
    mine = out.clone()
    d = v9.ResidDesc(v9.RESID_FORMATS["rgb_f16"], 2, 0, ow, oh, 0, 0)
    if L.vp9hip_residual_frames_scaled(dev._c, arr, n, ctypes.byref(d), mine.data_ptr(), stream) != 0:
        raise RuntimeError("vp9hip_residual_frames_scaled failed")
    torch.cuda.synchronize()
    err = float((mine.view(torch.float16).view(n, 3, oh, ow).float() - ref.float()).abs().max()) * m
    res["framework_max_diff_codes"] = err
    f = timed(framework, 3, args.framework_reps)
    res["framework"] = {"ms": f}
    for fmt in ("rgb_f16", "yuv_i16"):
        t = res[fmt]["ms"]["median"]
        res[fmt]["ratio_to_copy"] = c["median"] / t
        res[fmt]["ratio_to_framework"] = f["median"] / t
        res[fmt]["ratio_to_convert_scale"] = k["median"] / t
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--framework-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = v9.lib()
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    side = torch.cuda.Stream()                                 # a stream of torch's own: launches go to it directly
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream, "the timed stream must not be the null stream"
    res = {"tool": "residual_scale_bench", "device": v9.device_info(0)[1], "reps": args.reps,
           "cases": [case(L, stream, 3840, 2160, args.frames, 224, 224, args),
                     case(L, stream, 1920, 1080, args.frames, 224, 224, args)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
