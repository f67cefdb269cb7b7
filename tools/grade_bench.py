#!/usr/bin/env python3
"""Graded output (vp9hip_convert_frames_graded) beside the same call ungraded, timed as
tools/convert_bench.py times its cases: one launch over `--frames` frames per repetition between
two HIP events on a stream of torch's own, the median of `--reps`.

Two workloads at rgbp_f16 from 10-bit 3840x2160 frames of uniformly random samples (the worst case
for the tables' locality; pictures are smoother):
  A  -> 224x224, triangle filter: the grade runs on 50 K pixels per frame
  B  the visible size (the box filter at equal size): the grade's per-pixel cost
each graded (an HDR10 -> sRGB grade, make_grade(10, "rgbp_f16", "pq", "bt2020")), ungraded through
the same kernel, and as what a caller does without it: the ungraded call followed by the framework
composition on the half tensor (codes -> index gather -> 3x3 matmul in float -> clamp -> gather).
B also reports a device copy of its output, the cost of a second pass over it.

    python tools/grade_bench.py [--out profiles/NAME.json] [--lib path/to/libvp9hip.so]

--lib loads another build of the library (the A/B of a kernel variant). Prints one JSON line.
Needs a GPU; there is no fallback.
"""
import argparse
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
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.lib:
        v9.LIB_PATH = os.path.abspath(args.lib)
    w, h = (int(x) for x in args.size.split("x"))
    n, bpp, fmt = args.frames, 10, "rgbp_f16"
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    dev = v9.Device(0)
    dev.configure(w, h, bpp, nbufs=n)
    rng = np.random.default_rng(1)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    pictures = [[rng.integers(0, 1 << bpp, s).astype(np.uint16) for s in ((h, w), (ch, cw), (ch, cw))] for _ in range(2)]
    for b in range(n):              # two distinct random frames, alternating
        dev.upload(b, pictures[b % 2])
    dev.sync()
    host = v9.make_grade(bpp, fmt, "pq", "bt2020")
    g = dev.grade(host)
    in_t = torch.from_numpy(host.in_lut.astype(np.float32)).cuda()
    out_t = torch.from_numpy((host.out_lut.astype(np.float32) / 65535).astype(np.float16)).cuda()
    m_t = torch.from_numpy((host.m / 16384.0).astype(np.float32)).cuda()
    bufs = list(range(n))
    res = {"tool": "grade_bench", "size": [w, h], "frames": n, "reps": args.reps, "bpp": bpp, "format": fmt,
           "lib": v9.LIB_PATH if args.lib else "in-tree", "device": v9.device_info(0)[1], "cases": []}

    def framework(x):               # the ungraded half tensor (N, 3, H, W) -> the graded one, in framework kernels
        codes = (x.float() * 1023).round_().long()
        lin = in_t[codes]
        p = torch.einsum("rc,nchw->nrhw", m_t, lin).clamp_(0, 65535)
        return out_t[(p * (1 / 16)).long()]

    for name, kw, (ow, oh) in (("A: 224x224 triangle", dict(resize=(224, 224), filter="triangle"), (224, 224)),
                               ("B: visible size", dict(resize=(w, h), src_rects=(0, 0, w, h)), (w, h))):
        nbytes = n * v9.out_layout(fmt, ow, oh, bpp)[0]
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        e = {"case": name, "out": [ow, oh], "bytes_written": nbytes}
        e["ungraded_ms"] = timed(lambda: dev.convert(bufs, fmt, colorspace=5, out=out, **kw), args.warmup, args.reps)
        e["graded_ms"] = timed(lambda: dev.convert(bufs, fmt, colorspace=5, out=out, grade=g, **kw), args.warmup, args.reps)
        e["graded_to_ungraded"] = e["graded_ms"]["median"] / e["ungraded_ms"]["median"]
        try:
            e["ungraded_then_framework_ms"] = timed(lambda: framework(dev.convert(bufs, fmt, colorspace=5, out=out, **kw)),
                                                    max(2, args.warmup // 4), max(5, args.reps // 4))
            e["framework_to_graded"] = e["ungraded_then_framework_ms"]["median"] / e["graded_ms"]["median"]
        except RuntimeError as err:      # reported, not worked around: the yardstick is what it is
            e["ungraded_then_framework_error"] = str(err)[:300]
        if (ow, oh) == (w, h):
            dst = torch.empty_like(out)
            e["copy_of_output_ms"] = timed(lambda: dst.copy_(out), args.warmup, args.reps)
            e["grade_cost_to_copy_of_output"] = ((e["graded_ms"]["median"] - e["ungraded_ms"]["median"]) /
                                                 e["copy_of_output_ms"]["median"])
            del dst
        res["cases"].append(e)
        del out
        torch.cuda.empty_cache()
    g.close()
    dev.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
