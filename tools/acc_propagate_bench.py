#!/usr/bin/env python3
"""Accumulated propagation cost (k_prop_nchw / k_prop_nhwc, csrc/vp9hip_prop.hip) against a
device-to-device copy and against the framework composition.

`--pairs` pairs of a 3840x2160 field each, all reading one source item (the root frame's tensor),
through vp9hip_prop_launch_dev, with the valid map:
  labels-u8     a dense uint8 label map, C = 1 on 3840x2160, nearest
  labels-i64    an int64 label map on 512x512, nearest
  feat-f16-*    a float16 feature map, C = 256 on 240x135, NCHW and NHWC, nearest and bilinear
Two sets of fields: "zero" (every cell applies, all vectors zero: the gather is the identity) and
"gop" (a key frame and `--pairs` synthetic inter frames, vp9hip_synth_frame's defaults, each
following the one before it under every reference name; the fields are vp9hip_motion_acc_host's).
Every result is compared with vp9hip_acc_propagate_host first.

Each repetition runs between two HIP events on the launches' stream, medians with min - max: us,
and the ratio to the yardsticks, timed the same way in the same run:
  copy: a hipMemcpyAsync device-to-device copy of the bytes the definition moves, one source
    element read and one element written per output element, the fields read and the valid maps
    written; it copies half of them: every copied byte is read once and written once.
  torch: the framework composition over the same tensors: the cells widened to a sampling grid at
    the tensor's size, torch.nn.functional.grid_sample (border padding, nearest or bilinear) and
    the fill where the cell does not apply, labels through float and back. That composition is
    another function (float coordinates, float labels), so its result is not compared.

    python tools/acc_propagate_bench.py [--out profiles/NAME.json]

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

W, H = 3840, 2160
SHAPES = [("labels-u8", np.uint8, 1, (3840, 2160), "nchw", "nearest"),
          ("labels-i64", np.int64, 1, (512, 512), "nchw", "nearest"),
          ("feat-f16-nchw-nearest", np.float16, 256, (240, 135), "nchw", "nearest"),
          ("feat-f16-nchw-bilinear", np.float16, 256, (240, 135), "nchw", "bilinear"),
          ("feat-f16-nhwc-nearest", np.float16, 256, (240, 135), "nhwc", "nearest"),
          ("feat-f16-nhwc-bilinear", np.float16, 256, (240, 135), "nhwc", "bilinear")]


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


def us(t):
    return {"median": 1e3 * t[0], "min": 1e3 * t[1], "max": 1e3 * t[2]}


def gop_fields(n):
    """The accumulated fields of n inter frames chained onto a key frame of serial 100."""
    key = v9.SynthFrame(v9.synth_params(W, H, 8, seed=0x61770000, log2_tile_cols=2))
    prev = v9.motion_acc_host(*v9.motion_host(key), 100)
    out = []
    for i in range(n):
        f = v9.SynthFrame(v9.synth_params(W, H, 8, seed=0x61770001 + i, inter=1, log2_tile_cols=2))
        prev = v9.motion_acc_host(*v9.motion_host(f), 101 + i, [prev] * 3)
        out.append(prev)
    return out


def torch_composition(src, acc, serial, fw, fh, interp, layout, fill):
    """(n, ...) like src's item: grid_sample of the one source item through the cells' vectors
    widened to the fw x fh grid, the fill where the cell does not apply."""
    n = acc.shape[0]
    ys = (((2 * torch.arange(fh, device="cuda") + 1) * H) // (2 * fh)) >> 2
    xs = (((2 * torch.arange(fw, device="cuda") + 1) * W) // (2 * fw)) >> 2
    q = acc[:, ys][:, :, xs]                                    # cells to samples: (n, fh, fw, 4)
    app = ((q[..., 3] & 0xffff) > 0) & (q[..., 2] == serial)
    gy, gx = torch.meshgrid(torch.arange(fh, device="cuda", dtype=torch.float32),
                            torch.arange(fw, device="cuda", dtype=torch.float32), indexing="ij")
    gx = gx + q[..., 0].float() * (fw / (8.0 * W))
    gy = gy + q[..., 1].float() * (fh / (8.0 * H))
    grid = torch.stack((gx * (2.0 / max(fw - 1, 1)) - 1.0, gy * (2.0 / max(fh - 1, 1)) - 1.0), -1)
    x = src if src.dim() == 4 else src[:, None]
    if layout == "nhwc" and src.dim() == 4:
        x = x.permute(0, 3, 1, 2)
    x = x if x.dtype == torch.float16 else x.float()            # labels through float
    out = torch.nn.functional.grid_sample(x.expand(n, -1, -1, -1), grid.to(x.dtype), mode=interp, padding_mode="border",
                                          align_corners=True)
    out = torch.where(app[:, None], out, fill).to(src.dtype)
    if src.dim() == 3:
        return out[:, 0]
    return out.permute(0, 2, 3, 1).contiguous() if layout == "nhwc" else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--torch-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.pairs
    L = v9.lib()
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    res = {"tool": "acc_propagate_bench", "device": v9.device_info(0)[1], "reps": args.reps, "field": [W, H], "pairs": n, "cases": []}
    side = torch.cuda.Stream()                                 # a stream of torch's own: launches go to it directly
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream, "the timed stream must not be the null stream"
    gw, gh = 2 * ((W + 7) >> 3), 2 * ((H + 7) >> 3)
    zero = np.zeros((gh, gw), v9.ACC_CELL)
    zero["root"], zero["hops"] = 100, 1
    rng = np.random.default_rng(0x7072)
    for fname, fields in (("zero", [zero] * n), ("gop", gop_fields(n))):
        acc = torch.from_numpy(np.stack([f.view("<i4").reshape(gh, gw, 4) for f in fields])).cuda()
        ptrs = [acc[i].data_ptr() for i in range(n)]
        for name, dtype, C, (fw, fh), layout, interp in SHAPES:
            if dtype == np.float16:
                item = rng.integers(-2000, 2000, (C, fh, fw)).astype(np.float16)
            else:
                item = rng.integers(0, 200, (C, fh, fw)).astype(dtype)
            hsrc = np.ascontiguousarray(item.transpose(1, 2, 0)) if layout == "nhwc" else item
            if C == 1:
                hsrc = item[0]
            src = torch.from_numpy(hsrc[None]).cuda()
            dst = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device="cuda")
            valid = torch.empty((n, fh, fw), dtype=torch.uint8, device="cuda")
            E = src.element_size()
            d = v9.PropDesc(W, H, fw, fh, C, E, v9.PROP_LAYOUTS[layout], v9.WARP_MODES[interp], 0, 0, 0)

            def launch():
                v9.prop_launch_dev(ptrs, gw, [100] * n, [0] * n, 1, d, src.data_ptr(), dst.data_ptr(), valid.data_ptr(), stream)
            dst.view(torch.uint8).fill_(0x5a)
            valid.fill_(0x5a)
            launch()
            torch.cuda.synchronize()
            got, gv = dst.cpu().numpy(), valid.cpu().numpy()
            applying = 0.0
            for i in range(n):
                want, wv = v9.acc_propagate_host(fields[i], 100, hsrc, W, H, interp=interp, layout=layout, valid=True)
                if got[i].tobytes() != want.tobytes() or not np.array_equal(gv[i], wv):
                    raise RuntimeError("%s %s: pair %d differs from vp9hip_acc_propagate_host" % (name, fname, i))
                applying += float(wv.mean()) / n
            moved = n * (2 * C * fh * fw * E + fh * fw + 16 * gw * gh)
            a, b = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            a.fill_(0x33)

            def copy():
                if L.hipMemcpyAsync(b.data_ptr(), a.data_ptr(), moved // 2, 3, stream) != 0:    # hipMemcpyDeviceToDevice
                    raise RuntimeError("hipMemcpyAsync failed")
            t, c = timed(launch, args.warmup, args.reps), timed(copy, args.warmup, args.reps)
            fwk = timed(lambda: torch_composition(src, acc, 100, fw, fh, interp, layout, 0), 2, args.torch_reps)
            res["cases"].append({"shape": name, "fields": fname, "dtype": np.dtype(dtype).name, "channels": C, "grid": [fw, fh],
                                 "layout": layout, "interp": interp, "applying": applying, "bytes": moved, "us": us(t),
                                 "copy_us": us(c), "torch_us": us(fwk), "GBps": moved / (1e6 * t[0]),
                                 "ratio_to_copy": t[0] / c[0], "torch_over_kernel": fwk[0] / t[0]})
            del a, b, dst, valid, src
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
