#!/usr/bin/env python3
"""Accumulated residual cost (k_acc_warp, csrc/vp9hip_warp.hip) against a device-to-device copy
and against the framework composition.

`--pairs` pairs (frame i, the root frame) of 3840x2160 and of 1920x1080, 8-bit 4:2:0, random
pictures in buffers of the library's layout (pitch a multiple of 64 samples), through
vp9hip_warp_launch_dev: both modes, residual output, with and without the mask. Two sets of
fields: "zero" (every cell applies, all vectors zero: the gather is the identity) and "gop" (a
key frame and `--pairs` synthetic inter frames, vp9hip_synth_frame's defaults, each following
the one before it under every reference name; the fields are vp9hip_motion_acc_host's, so the
vectors and the cells that still reach the root are drawn as the GOP chains draw them). Every
result is compared with vp9hip_acc_warp_host first.

Each repetition runs between two HIP events on the launches' stream, medians with min - max: us,
and the ratio to the yardsticks, timed the same way in the same run:
  copy: a hipMemcpyAsync device-to-device copy of the bytes the definition moves, a read + b read
    + acc read + output written (+ the mask); it copies half of them: every copied byte is read
    once and written once.
  torch: the framework composition over the same tensors: the cells' vectors widened to a
    per-sample grid, torch.nn.functional.grid_sample (float, border padding), subtract, mask by
    the applying cells, to int16, for the three planes. A float bilinear is another function, so
    its result is not compared.

    python tools/acc_warp_bench.py [--out profiles/NAME.json]

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


def gop_fields(w, h, log2, n):
    """The accumulated fields of n inter frames chained onto a key frame of serial 100."""
    key = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x61770000, log2_tile_cols=log2))
    prev = v9.motion_acc_host(*v9.motion_host(key), 100)
    out = []
    for i in range(n):
        f = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x61770001 + i, inter=1, log2_tile_cols=log2))
        prev = v9.motion_acc_host(*v9.motion_host(f), 101 + i, [prev] * 3)
        out.append(prev)
    return out


def torch_composition(a_pl, b_pl, acc, sb, sizes, subs, interp):
    """(y, u, v) int16: a - grid_sample(b) where the cell applies, else 0; N pairs at once."""
    app = ((acc[..., 3] & 0xffff) > 0) & (acc[..., 2] == sb)
    out = []
    for a, b, (pw, ph), (sh, sv) in zip(a_pl, b_pl, sizes, subs):
        def wide(t):                                           # cells to samples of this plane
            return t.repeat_interleave(4 >> sv, 1).repeat_interleave(4 >> sh, 2)[:, :ph, :pw]
        ys, xs = torch.meshgrid(torch.arange(ph, device="cuda", dtype=torch.float32),
                                torch.arange(pw, device="cuda", dtype=torch.float32), indexing="ij")
        gx = xs + wide(acc[..., 0].float()) * (1.0 / (8 << sh))
        gy = ys + wide(acc[..., 1].float()) * (1.0 / (8 << sv))
        grid = torch.stack((gx * (2.0 / max(pw - 1, 1)) - 1.0, gy * (2.0 / max(ph - 1, 1)) - 1.0), -1)
        pred = torch.nn.functional.grid_sample(b[:, None, :ph, :pw].float(), grid, mode=interp, padding_mode="border",
                                               align_corners=True)[:, 0]
        out.append(torch.where(wide(app), a[:, :ph, :pw].float() - pred, 0.0).round().to(torch.int16))
    return out


def size_cases(L, stream, w, h, log2, n, args):
    cw, ch, gw, gh = (w + 1) >> 1, (h + 1) >> 1, 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)
    pitch = ((w + 63) // 64 * 64, (w + 63) // 64 * 64 // 2)
    off = (0, pitch[0] * h, pitch[0] * h + pitch[1] * ch)
    rng = np.random.default_rng(0x6177)
    frames = torch.from_numpy(rng.integers(0, 256, (n + 1, off[2] + pitch[1] * ch), dtype=np.uint8)).cuda()   # 0: the root
    planes = [frames.as_strided((n + 1, ch if p else h, pitch[1 if p else 0]), (frames.stride(0), pitch[1 if p else 0], 1), off[p])
              for p in range(3)]
    host = [[pl[i].cpu().numpy() for pl in planes] for i in range(n + 1)]
    sizes, subs = ((w, h), (cw, ch), (cw, ch)), ((0, 0), (1, 1), (1, 1))
    stride, doff = v9.warp_layout(w, h)
    dst = torch.empty(n * stride // 2, dtype=torch.int16, device="cuda")
    mask = torch.empty((n, gh, gw), dtype=torch.uint8, device="cuda")
    zero = np.zeros((gh, gw), v9.ACC_CELL)
    zero["root"], zero["hops"] = 100, 1
    out = []
    for name, fields in (("zero", [zero] * n), ("gop", gop_fields(w, h, log2, n))):
        acc = torch.from_numpy(np.stack([f.view("<i4").reshape(gh, gw, 4) for f in fields])).cuda()
        app = float(np.mean([((f["hops"] > 0) & (f["root"] == 100)).mean() for f in fields]))
        ptr = lambda v: (ctypes.c_void_p * n)(*v)   # noqa: E731
        a_p, b_p = ptr([frames[i + 1].data_ptr() for i in range(n)]), ptr([frames[0].data_ptr()] * n)
        c_p, ser = ptr([acc[i].data_ptr() for i in range(n)]), (ctypes.c_uint32 * n)(*[100] * n)
        c_off, c_pitch = (ctypes.c_int64 * 3)(*off), (ctypes.c_int32 * 2)(*pitch)
        moved = n * (2 * (w * h + 2 * cw * ch) + 16 * gw * gh + stride)
        res = {"size": [w, h], "pairs": n, "fields": name, "applying": app, "bytes": moved, "runs": {}}
        half = (moved + n * gw * gh) // 2
        src, cpy = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        src.fill_(0x33)
        for interp in ("nearest", "bilinear"):
            for with_mask in (False, True):
                def launch():
                    if L.vp9hip_warp_launch_dev(a_p, b_p, c_p, ser, n, ctypes.byref(c_off), ctypes.byref(c_pitch), gw, w, h, 8, 1, 1,
                                                v9.WARP_MODES[interp], 0, dst.data_ptr(), mask.data_ptr() if with_mask else None,
                                                stream) != 0:
                        raise RuntimeError("vp9hip_warp_launch_dev failed")
                dst.fill_(0x5a5a)
                mask.fill_(0x5a)
                launch()
                torch.cuda.synchronize()
                got, gm = dst.cpu().numpy().reshape(n, stride // 2), mask.cpu().numpy()
                for i in range(n if not with_mask else 1):     # the mask runs differ only in the mask: one pair's planes
                    want = v9.acc_warp_host(host[i + 1], host[0], fields[i], 100, w, h, 8, interp=interp, mask=True)
                    for p, (pw, ph) in enumerate(sizes):
                        if not np.array_equal(got[i, doff[p] // 2:doff[p] // 2 + pw * ph].reshape(ph, pw), want[p]):
                            raise RuntimeError("%dx%d %s %s: pair %d plane %d differs from vp9hip_acc_warp_host" % (w, h, name, interp, i, p))
                if with_mask:
                    for i in range(n):
                        if not np.array_equal(gm[i], ((fields[i]["hops"] > 0) & (fields[i]["root"] == 100)).astype(np.uint8)):
                            raise RuntimeError("%dx%d %s: pair %d's mask differs" % (w, h, name, i))
                nbytes = moved + (n * gw * gh if with_mask else 0)

                def copy():
                    if L.hipMemcpyAsync(cpy.data_ptr(), src.data_ptr(), nbytes // 2, 3, stream) != 0:    # hipMemcpyDeviceToDevice
                        raise RuntimeError("hipMemcpyAsync failed")
                t, c = timed(launch, args.warmup, args.reps), timed(copy, args.warmup, args.reps)
                run = {"us": us(t), "copy_us": us(c), "ratio_to_copy": t[0] / c[0], "bytes": nbytes,
                       "GBps": nbytes / (1e6 * t[0])}
                if not with_mask:
                    fw = timed(lambda: torch_composition([pl[1:] for pl in planes], [pl[:1].expand(n, -1, -1) for pl in planes],
                                                         acc, 100, sizes, subs, interp), 3, args.torch_reps)
                    run.update(torch_us=us(fw), torch_over_kernel=fw[0] / t[0])
                res["runs"]["%s%s" % (interp, ", mask" if with_mask else "")] = run
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--torch-reps", type=int, default=20)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = v9.lib()
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    res = {"tool": "acc_warp_bench", "device": v9.device_info(0)[1], "reps": args.reps, "cases": []}
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
