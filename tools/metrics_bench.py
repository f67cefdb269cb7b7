#!/usr/bin/env python3
"""Frame metrics cost (k_metrics, csrc/vp9hip_metrics.hip) against two yardsticks timed in the
same run, in one process, on a side stream of torch's.

Cases: `--pairs` pairs of 3840x2160 8-bit, 3840x2160 10-bit and 1920x1080 8-bit frames (random
codes over the whole range, 2 x pairs distinct buffers), each with and without the cell map. The
outputs of both variants, all pairs, are first compared with vp9hip_frame_metrics_host. Each
repetition is timed between two HIP events on the launch's stream; medians with min / max.

  (a) copy: a hipMemcpyAsync device-to-device copy of as many bytes as the launch reads. The
      copy also writes that much, so a read-only pass at the same read rate has about 2 x
      headroom.
  (b) framework: the same buffers through frame_tensors views: widen to int32, subtract, then
      abs().sum() and square().sum() per plane (SAD and SSE only, a fraction of the record).

Reported: the launch in us and GB/s over the bytes read, and the ratios to (a) and (b) (above 1:
the launch is faster).

    python tools/metrics_bench.py [--out profiles/NAME.json]

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
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def case(L, stream, w, h, bpp, n, args):
    rng = np.random.default_rng(w + bpp)
    dt = np.uint8 if bpp == 8 else np.uint16
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    dev = v9.Device(0)
    dev.configure(w, h, bpp, nbufs=2 * n)
    host = [[rng.integers(0, 1 << bpp, s).astype(dt) for s in ((h, w), (ch, cw), (ch, cw))] for _ in range(4)]
    for b in range(2 * n):
        dev.upload(b, host[b % 4])
    ba, bb = list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2))
    read = 2 * n * (w * h + 2 * cw * ch) * (1 if bpp == 8 else 2)
    out = torch.empty(n * 24, dtype=torch.int64, device="cuda")
    res = {"size": [w, h], "bpp": bpp, "pairs": n, "bytes_read": read}
    # correctness first: every pair of both timed variants against the host statement of the
    # definition (the pairs repeat two combinations of host frames)
    want = {}
    for i in range(n):
        key = (ba[i] % 4, bb[i] % 4)
        if key not in want:
            want[key] = v9.frame_metrics_host(host[key[0]], host[key[1]], w, h, bpp, cells=True)
    mh, mw = (h + 15) >> 4, (w + 15) >> 4
    cells = torch.empty((n, mh, mw), dtype=torch.int32, device="cuda")
    m = out.view(n, 3, 8)
    aa, ab = (ctypes.c_int * n)(*ba), (ctypes.c_int * n)(*bb)
    for name, cptr in (("metrics", None), ("metrics_and_map", cells.data_ptr())):
        def launch():
            if L.vp9hip_frame_metrics(dev._c, aa, ab, n, w, h, out.data_ptr(), cptr, stream) != 0:
                raise RuntimeError("vp9hip_frame_metrics failed")
        out.fill_(0x55)
        cells.fill_(0x55)
        launch()
        torch.cuda.synchronize()
        gm, gc = m.cpu().numpy(), cells.cpu().numpy()
        for i in range(n):
            wm, wc = want[(ba[i] % 4, bb[i] % 4)]
            if not (np.array_equal(gm[i], wm) and (cptr is None or np.array_equal(gc[i], wc))):
                raise RuntimeError("%dx%d %d-bit %s: pair %d differs from vp9hip_frame_metrics_host" % (w, h, bpp, name, i))
        t = timed(launch, args.warmup, args.reps)
        res[name] = {"ms": t, "us": 1e3 * t["median"], "GBps": read / t["median"] / 1e6}
    # (a) a device-to-device copy of the bytes the launch reads
    src = torch.empty(read, dtype=torch.uint8, device="cuda")
    dst = torch.empty(read, dtype=torch.uint8, device="cuda")
    src.fill_(0x33)

    def copy():
        if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), read, 3, stream) != 0:    # hipMemcpyDeviceToDevice
            raise RuntimeError("hipMemcpyAsync failed")
    c = timed(copy, args.warmup, args.reps)
    res["copy"] = {"ms": c, "GBps_read": read / c["median"] / 1e6}
    del src, dst
    # (b) the framework route on the same buffers
    views = [dev.frame_tensors(b) for b in range(2 * n)]

    def framework():
        r = []
        for x, y in zip(ba, bb):
            for p in range(3):
                d = views[x][p].to(torch.int32) - views[y][p].to(torch.int32)
                r.append((d.abs().sum(), d.square().sum()))
        return r
    got = framework()
    torch.cuda.synchronize()
    if int(got[0][0]) != int(m[0, 0, 3]) or int(got[0][1]) != int(m[0, 0, 4]):
        raise RuntimeError("the framework route disagrees on pair 0's luma SAD / SSE")
    f = timed(framework, 3, args.framework_reps)
    res["framework"] = {"ms": f}
    for name in ("metrics", "metrics_and_map"):
        res[name]["ratio_to_copy"] = c["median"] / res[name]["ms"]["median"]
        res[name]["ratio_to_framework"] = f["median"] / res[name]["ms"]["median"]
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
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
    res = {"tool": "metrics_bench", "device": v9.device_info(0)[1], "reps": args.reps,
           "cases": [case(L, stream, 3840, 2160, 8, args.pairs, args), case(L, stream, 3840, 2160, 10, args.pairs, args),
                     case(L, stream, 1920, 1080, 8, args.pairs, args)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
