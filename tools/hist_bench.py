#!/usr/bin/env python3
"""Frame histogram cost (k_hist, csrc/vp9hip_hist.hip) against two yardsticks timed in the same
run, in one process, on a side stream of torch's.

Cases: `--frames` frames of 3840x2160 8-bit, 3840x2160 10-bit and 1920x1080 8-bit (4:2:0, that many
distinct buffers), each with three contents:
  noise     uniform codes over the whole range, every plane;
  constant  one code a plane (luma 16 << (bpp - 8), chroma mid): the worst case of the LDS atomics;
  content   a stand-in with the statistics of decoded video: a smooth diagonal ramp plus +-2 codes
            of noise, a constant 12.5 % bar top and bottom, chroma likewise around mid.
and three launches: PLANES with 256 bins, PLANES with one bin per code, RGBM with one bin per code
(BT.709, limited range). Every output, all frames, is first compared with
vp9hip_frame_histograms_host. Each repetition is timed between two HIP events on the launch's
stream; medians with min / max.

  (a) copy: a hipMemcpyAsync device-to-device copy of as many bytes as the launch reads. The copy
      also writes that much, so a read-only pass at the same read rate has about 2 x headroom.
  (b) framework: torch.bincount(plane.reshape(-1).to(int32) >> shift, minlength=B) on the
      frame_tensors views, per plane and frame (the widening is what bincount needs for the int16
      storage; at 8 bits uint8 goes in as it is where no shift is needed). PLANES only: RGBM has
      no framework route short of a full-size conversion, so it is reported beside
  (c) convert: Device.convert(bufs, "rgbp_f16") of the same frames at full size.

Reported: each launch in us and GB/s over the bytes read, its ratios to (a), (b) and (c) (above 1:
the launch is faster), and per launch the constant / noise time ratio, the measure of the
contention countermeasure.

    python tools/hist_bench.py [--out profiles/NAME.json]

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

DISTINCT = 2                                                     # distinct host frames a content; the buffers repeat them


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


def make(content, rng, w, h, bpp):
    dt = np.uint8 if bpp == 8 else np.uint16
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    top, up = (1 << bpp) - 1, 1 << (bpp - 8)
    shapes = ((h, w), (ch, cw), (ch, cw))
    if content == "noise":
        return [rng.integers(0, 1 << bpp, s).astype(dt) for s in shapes]
    if content == "constant":
        return [np.full(s, (16 if p == 0 else 128) * up, dt) for p, s in enumerate(shapes)]
    out = []
    for p, (ph, pw) in enumerate(shapes):
        yy, xx = np.mgrid[:ph, :pw]
        base = (16 * up + (xx * 3 + yy * 2) * (200 * up) // (3 * pw + 2 * ph)) if p == 0 else \
               (128 * up + ((xx - yy) * (30 * up)) // (pw + ph))
        a = np.clip(base + rng.integers(-2, 3, (ph, pw)), 0, top)
        bar = ph // 8
        a[:bar] = a[ph - bar:] = (16 if p == 0 else 128) * up
        out.append(a.astype(dt))
    return out


def case(L, stream, w, h, bpp, n, args):
    rng = np.random.default_rng(w + bpp)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    dev = v9.Device(0)
    dev.configure(w, h, bpp, nbufs=n)
    read = n * (w * h + 2 * cw * ch) * (1 if bpp == 8 else 2)
    res = {"size": [w, h], "bpp": bpp, "frames": n, "bytes_read": read, "contents": {}}
    bufs = list(range(n))
    arr = (ctypes.c_int * n)(*bufs)
    launches = [("planes_256", "planes", 256), ("planes_full", "planes", 1 << bpp), ("rgbm_full", "rgbm", 1 << bpp)]
    out = torch.empty(n * 4 << bpp, dtype=torch.int32, device="cuda")
    # (a) a device-to-device copy of the bytes a launch reads
    src = torch.empty(read, dtype=torch.uint8, device="cuda")
    dst = torch.empty(read, dtype=torch.uint8, device="cuda")
    src.fill_(0x33)

    def copy():
        if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), read, 3, stream) != 0:    # hipMemcpyDeviceToDevice
            raise RuntimeError("hipMemcpyAsync failed")
    c = timed(copy, args.warmup, args.reps)
    res["copy"] = {"ms": c, "GBps_read": read / c["median"] / 1e6}
    del src, dst
    views = [dev.frame_tensors(b) for b in bufs]
    for content in ("noise", "constant", "content"):
        host = [make(content, rng, w, h, bpp) for _ in range(DISTINCT)]
        for b in bufs:
            dev.upload(b, host[b % DISTINCT])
        dev.sync()
        r = {}
        for name, what, bins in launches:
            C = 3 if what == "planes" else 4
            d = v9.HistDesc(v9.HIST_MODES[what], bins.bit_length() - 1, 2, 0, w, h, None)
            res_view = out[:n * C * bins].view(n, C, bins)

            def launch():
                if L.vp9hip_frame_histograms(dev._c, arr, n, ctypes.byref(d), out.data_ptr(), stream) != 0:
                    raise RuntimeError("vp9hip_frame_histograms failed")
            # correctness first: every frame against the host statement of the definition
            out.fill_(0x55)
            launch()
            torch.cuda.synchronize()
            got = res_view.cpu().numpy()
            want = [v9.histograms_host(p, w, h, bpp, what=what, bins=bins) for p in host]
            for i in range(n):
                if not np.array_equal(got[i], want[i % DISTINCT]):
                    raise RuntimeError("%dx%d %d-bit %s %s: frame %d differs from vp9hip_frame_histograms_host"
                                       % (w, h, bpp, content, name, i))
            t = timed(launch, args.warmup, args.reps)
            r[name] = {"ms": t, "us": 1e3 * t["median"], "GBps": read / t["median"] / 1e6,
                       "ratio_to_copy": c["median"] / t["median"]}
        # (b) the framework route on the same buffers, PLANES
        for name, bins in (("planes_256", 256), ("planes_full", 1 << bpp)):
            sh = bpp - (bins.bit_length() - 1)

            def framework():
                tabs = []
                for b in bufs:
                    for p in range(3):
                        x = views[b][p].reshape(-1)
                        if bpp > 8 or sh:
                            x = x.to(torch.int32) >> sh
                        tabs.append(torch.bincount(x, minlength=bins))
                return tabs
            tabs = framework()
            torch.cuda.synchronize()
            ref = v9.histograms_host(host[0], w, h, bpp, bins=bins)
            if not all(np.array_equal(tabs[p].cpu().numpy(), ref[p]) for p in range(3)):
                raise RuntimeError("the framework route disagrees on frame 0")
            f = timed(framework, 3, args.framework_reps)
            r[name]["framework_ms"] = f
            r[name]["ratio_to_framework"] = f["median"] / r[name]["ms"]["median"]
        # (c) the full-size conversion, beside RGBM
        cvt_out = torch.empty(n * v9.out_layout("rgbp_f16", w, h, bpp)[0], dtype=torch.uint8, device="cuda")
        cv = timed(lambda: dev.convert(bufs, "rgbp_f16", out=cvt_out, stream=stream), 3, args.framework_reps)
        del cvt_out
        r["rgbm_full"]["convert_rgbp_f16_ms"] = cv
        r["rgbm_full"]["ratio_to_convert"] = cv["median"] / r["rgbm_full"]["ms"]["median"]
        r["rgbm_full"]["ratio_to_planes_full"] = r["rgbm_full"]["ms"]["median"] / r["planes_full"]["ms"]["median"]
        res["contents"][content] = r
    res["constant_over_noise"] = {name: res["contents"]["constant"][name]["ms"]["median"] /
                                  res["contents"]["noise"][name]["ms"]["median"] for name, _, _ in launches}
    res["content_over_noise"] = {name: res["contents"]["content"][name]["ms"]["median"] /
                                 res["contents"]["noise"][name]["ms"]["median"] for name, _, _ in launches}
    del views
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--framework-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = v9.lib()
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    side = torch.cuda.Stream()                                 # a stream of torch's own: launches go to it directly
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream, "the timed stream must not be the null stream"
    res = {"tool": "hist_bench", "device": v9.device_info(0)[1], "reps": args.reps,
           "cases": [case(L, stream, 3840, 2160, 8, args.frames, args), case(L, stream, 3840, 2160, 10, args.frames, args),
                     case(L, stream, 1920, 1080, 8, args.frames, args)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
