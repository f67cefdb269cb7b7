#!/usr/bin/env python3
"""Accumulated residual at model size (k_acc_warp_scale, csrc/vp9hip_warp_scale.hip): its cost
against a device-to-device copy, against k_acc_warp alone, and against today's whole route.

`--pairs` pairs (frame i, the root frame) of 3840x2160 and of 1920x1080, 8-bit 4:2:0, random
pictures in buffers of the library's layout (pitch a multiple of 64 samples), through
vp9hip_warp_scale_launch_dev to 224 x 224 "rgb_f16": both modes, with and without the coverage
plane, on the two sets of fields of tools/acc_warp_bench.py ("zero": every cell applies, all
vectors zero; "gop": a key frame and `--pairs` synthetic inter frames chained onto it). Every
result is compared with vp9hip_acc_warp_scaled_host first.

One process, a side stream of torch's own, `--warmup` launches, then `--reps` repetitions each
between two HIP events: medians with min - max, in us. Yardsticks, timed the same way in the same
run:
  (a) copy: a hipMemcpyAsync device-to-device copy of the bytes the definition moves (a + b +
      field read, the small output written); it copies half of them: every copied byte is read
      once and written once.
  (b) acc_warp: k_acc_warp alone on the same inputs through vp9hip_warp_launch_dev, residual
      output, no mask: the first half of the route without this kernel.
  (c) route: (b), then the framework composition of DESIGN.md 15a over its planes: widen, upsample
      chroma, the float matrix, interpolate(mode="area"), half. Another function (no defined
      rounding), so its result is not compared.

    python tools/acc_warp_scale_bench.py [--out profiles/NAME.json]

Prints one JSON line. Needs a GPU; there is no fallback.
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch  # before the library: they share libamdhip64 (see _torch_first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
v9 = importlib.import_module("ffmpeg-hybrid_amd")
from acc_warp_bench import gop_fields, timed, us  # noqa: E402

KR, KB = 0.2126, 0.0722                                        # BT.709, limited range: colorspace 2


def size_cases(L, stream, w, h, log2, n, args):
    ow, oh = args.out_size
    cw, ch, gw, gh = (w + 1) >> 1, (h + 1) >> 1, 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)
    pitch = ((w + 63) // 64 * 64, (w + 63) // 64 * 64 // 2)
    off = (0, pitch[0] * h, pitch[0] * h + pitch[1] * ch)
    rng = np.random.default_rng(0x6177)
    frames = torch.from_numpy(rng.integers(0, 256, (n + 1, off[2] + pitch[1] * ch), dtype=np.uint8)).cuda()   # 0: the root
    planes = [frames.as_strided((n + 1, ch if p else h, pitch[1 if p else 0]), (frames.stride(0), pitch[1 if p else 0], 1), off[p])
              for p in range(3)]
    host = [[pl[i].cpu().numpy() for pl in planes] for i in range(n + 1)]
    wstride, doff = v9.warp_layout(w, h)
    full = torch.empty(n * wstride // 2, dtype=torch.int16, device="cuda")             # k_acc_warp's output: (b), (c)
    fy, fu, fv = (full.as_strided((n, ph, pw), (wstride // 2, pw, 1), o // 2)
                  for o, (pw, ph) in zip(doff, ((w, h), (cw, ch), (cw, ch))))
    dst = torch.empty(n * 4 * oh * ow, dtype=torch.float16, device="cuda")
    zero = np.zeros((gh, gw), v9.ACC_CELL)
    zero["root"], zero["hops"] = 100, 1
    sy, sc, kg = 255 / 219., 255 / 224., 1. - KR - KB
    mat = torch.tensor([[sy, 0., 2. * (1. - KR) * sc], [sy, -2. * KB * (1. - KB) / kg * sc, -2. * KR * (1. - KR) / kg * sc],
                        [sy, 2. * (1. - KB) * sc, 0.]], dtype=torch.float32, device="cuda") / 255
    out = []
    for name, fields in (("zero", [zero] * n), ("gop", gop_fields(w, h, log2, n))):
        acc = torch.from_numpy(np.stack([f.view("<i4").reshape(gh, gw, 4) for f in fields])).cuda()
        app = float(np.mean([((f["hops"] > 0) & (f["root"] == 100)).mean() for f in fields]))
        ptr = lambda v: (ctypes.c_void_p * n)(*v)   # noqa: E731
        a_p, b_p = ptr([frames[i + 1].data_ptr() for i in range(n)]), ptr([frames[0].data_ptr()] * n)
        c_p, ser = ptr([acc[i].data_ptr() for i in range(n)]), (ctypes.c_uint32 * n)(*[100] * n)
        c_off, c_pitch = (ctypes.c_int64 * 3)(*off), (ctypes.c_int32 * 2)(*pitch)
        read = n * (2 * (w * h + 2 * cw * ch) + 16 * gw * gh)
        res = {"size": [w, h], "out": [ow, oh], "pairs": n, "fields": name, "applying": app, "runs": {}}
        for interp in ("nearest", "bilinear"):
            mode = v9.WARP_MODES[interp]

            def warp():
                if L.vp9hip_warp_launch_dev(a_p, b_p, c_p, ser, n, ctypes.byref(c_off), ctypes.byref(c_pitch), gw, w, h, 8, 1, 1,
                                            mode, 0, full.data_ptr(), None, stream) != 0:
                    raise RuntimeError("vp9hip_warp_launch_dev failed")

            def route():
                warp()
                uv = torch.nn.functional.interpolate(torch.stack([fu, fv], 1).float(), scale_factor=2, mode="nearest")[:, :, :h, :w]
                rgb = torch.einsum("rc,nchw->nrhw", mat, torch.cat([fy.float()[:, None], uv], 1))
                return torch.nn.functional.interpolate(rgb, size=(oh, ow), mode="area").half()
            tb = timed(warp, args.warmup, args.reps)
            tc = timed(route, 3, args.framework_reps)
            want = None
            for cov in (True, False):
                P = 4 if cov else 3
                d = v9.WarptDesc(v9.RESID_FORMATS["rgb_f16"], 2, 0, mode, P, w, h, ow, oh, 0, 0)

                def launch():
                    if L.vp9hip_warp_scale_launch_dev(a_p, b_p, c_p, ser, n, ctypes.byref(c_off), ctypes.byref(c_pitch), gw, 8, 1, 1,
                                                      ctypes.byref(d), dst.data_ptr(), stream) != 0:
                        raise RuntimeError("vp9hip_warp_scale_launch_dev failed")
                dst.fill_(7.0)
                launch()
                torch.cuda.synchronize()
                got = dst.cpu().numpy()[:n * P * oh * ow].reshape(n, P, oh, ow)
                if want is None:                               # with the coverage first: its three planes serve the run without
                    want = np.stack([v9.acc_warp_scaled_host(host[i + 1], host[0], fields[i], 100, w, h, 8, 1, 1, "rgb_f16", (ow, oh),
                                                             interp=interp, coverage=True) for i in range(n)])
                if not np.array_equal(got.view(np.int16), want[:, :P].view(np.int16)):
                    raise RuntimeError("%dx%d %s %s: differs from vp9hip_acc_warp_scaled_host" % (w, h, name, interp))
                nbytes = read + n * P * oh * ow * 2
                src, cpy = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
                src.fill_(0x33)

                def copy():
                    if L.hipMemcpyAsync(cpy.data_ptr(), src.data_ptr(), nbytes // 2, 3, stream) != 0:    # hipMemcpyDeviceToDevice
                        raise RuntimeError("hipMemcpyAsync failed")
                t, c = timed(launch, args.warmup, args.reps), timed(copy, args.warmup, args.reps)
                res["runs"]["%s%s" % (interp, ", coverage" if cov else "")] = {
                    "us": us(t), "copy_us": us(c), "ratio_to_copy": t[0] / c[0], "bytes": nbytes, "GBps": nbytes / (1e6 * t[0]),
                    "acc_warp_us": us(tb), "acc_warp_bytes": read + n * wstride, "ratio_to_acc_warp": t[0] / tb[0],
                    "route_us": us(tc), "route_over_kernel": tc[0] / t[0]}
                del src, cpy
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--framework-reps", type=int, default=20)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--out-size", default="224x224", type=lambda s: tuple(int(x) for x in s.split("x")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = v9.lib()
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    res = {"tool": "acc_warp_scale_bench", "device": v9.device_info(0)[1], "reps": args.reps, "cases": []}
    side = torch.cuda.Stream()                                 # a stream of torch's own: launches go to it directly
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream, "the timed stream must not be the null stream"
    for s in args.sizes.split(","):
        w, h = (int(x) for x in s.split("x"))
        res["cases"] += size_cases(L, stream, w, h, 2 if w > 2048 else 0, args.pairs, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
