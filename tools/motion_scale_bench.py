#!/usr/bin/env python3
"""Motion tensors at model size (k_motion_scale, csrc/vp9hip_motion_scale.hip) against two
yardsticks timed in the same run, in one process, on a side stream of torch's.

Cases: `--frames` fields of 3840x2160 and of 1920x1080 to 224x224, from the motion field
("coded") and from the accumulated field ("acc"), as "f16" with the coverage plane (P = 3). A
field is the field of a decoded synthetic keyframe overwritten through Device.motion's /
Device.motion_acc's views with random vectors in [-1024, 1023] (1/8 pel), a quarter of the cells
intra, every second vector poison (two distinct fields, alternating over the buffers). The
outputs of every frame are first compared with vp9hip_motion_scaled_host. Each repetition is
timed between two HIP events on the launch's stream; medians with min / max.

  (a) copy: a hipMemcpyAsync device-to-device copy of the bytes the launch reads (the visible
      cells: 12 bytes a cell coded, 16 acc) plus those it writes.
  (b) framework: the same fields through the views: mask by the info plane (or hops), widen to
      float, expand every cell to 4x4 pixels, crop to the visible size,
      interpolate(mode="area"), scale, half. Its largest deviation from the definition is
      reported in the output's own units (output pixels; the coverage 0..1).

Reported: the launch in us and GB/s over the bytes read, and the ratios to (a) and (b) (above 1:
the launch is faster).

    python tools/motion_scale_bench.py [--out profiles/NAME.json]

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


def random_fields(rng, gw, gh):
    mv = rng.integers(-1024, 1024, (gh, gw, 2, 2)).astype(np.int16)
    mv[:, :, 1] = 0x7fff
    info = rng.integers(0, 3, (gh, gw, 4)).astype(np.uint8)
    intra = rng.random((gh, gw)) < 0.25
    info[..., 0][intra] = 255
    acc = np.zeros((gh, gw), v9.ACC_CELL)
    acc["dx"], acc["dy"] = mv[:, :, 0, 0], mv[:, :, 0, 1]
    acc["root"], acc["hops"] = 1, np.where(intra, 0, rng.integers(1, 9, (gh, gw)))
    return mv, info, acc


def case(L, stream, w, h, n, ow, oh, args):
    rng = np.random.default_rng(w)
    gw, gh = 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)
    cells = ((w + 3) >> 2) * ((h + 3) >> 2)
    dev = v9.Device(0)
    dev.set_export(motion=True, motion_acc=True)
    dev.configure(w, h, 8, nbufs=n)
    dev.set_timing(False)
    key = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x17c00))
    for b in range(n):
        dev.submit(key, b)
    dev.sync()
    host = [random_fields(rng, gw, gh) for _ in range(2)]
    for b in range(n):
        mv, info, acc = host[b % 2]
        vmv, vinfo = dev.motion(b)
        vmv.copy_(torch.from_numpy(mv))
        vinfo.copy_(torch.from_numpy(info))
        dev.motion_acc(b).copy_(torch.from_numpy(acc.view("<i4").reshape(gh, gw, 4)))
    torch.cuda.synchronize()
    written = n * 3 * ow * oh * 2
    res = {"size": [w, h], "grid": [gw, gh], "out": [ow, oh], "frames": n, "format": "f16", "planes": 3,
           "bytes_written": written}
    arr = (ctypes.c_int * n)(*range(n))
    out = torch.empty(n * 3 * oh * ow, dtype=torch.float16, device="cuda")
    kx, ky = ow / (8.0 * w), oh / (8.0 * h)
    scale = torch.tensor([kx, ky, 1.0 / 256], dtype=torch.float32, device="cuda")[None, :, None, None]
    for source in ("coded", "acc"):
        read = n * cells * (12 if source == "coded" else 16)
        d = v9.MvtDesc(v9.MVT_FORMATS["f16"], v9.MVT_SOURCES[source], 3, w, h, ow, oh, 0, 0)

        def launch():
            if L.vp9hip_motion_frames_scaled(dev._c, arr, n, ctypes.byref(d), out.data_ptr(), stream) != 0:
                raise RuntimeError("vp9hip_motion_frames_scaled failed")
        # correctness first: every frame against the host statement of the definition
        want = [v9.motion_scaled_host(mv, info, w, h, "f16", (ow, oh), source=source, acc=acc, mask=True).view(np.int16)
                for mv, info, acc in host]
        out.fill_(85.0)
        launch()
        torch.cuda.synchronize()
        got = out.view(torch.int16).cpu().numpy().reshape(n, 3, oh, ow)
        for i in range(n):
            if not np.array_equal(got[i], want[i % 2]):
                raise RuntimeError("%dx%d %s: frame %d differs from vp9hip_motion_scaled_host" % (w, h, source, i))
        t = timed(launch, args.warmup, args.reps)
        r = {"bytes_read": read, "ms": t, "us": 1e3 * t["median"], "GBps": read / t["median"] / 1e6}
        mine = out.view(n, 3, oh, ow).float().clone()
        # (a) a device-to-device copy of the bytes the launch reads plus those it writes
        src = torch.empty(read + written, dtype=torch.uint8, device="cuda")
        dst = torch.empty(read + written, dtype=torch.uint8, device="cuda")
        src.fill_(0x33)

        def copy():
            if L.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), read + written, 3, stream) != 0:    # hipMemcpyDeviceToDevice
                raise RuntimeError("hipMemcpyAsync failed")
        c = timed(copy, args.warmup, args.reps)
        r["copy"] = {"ms": c, "GBps": (read + written) / c["median"] / 1e6}
        del src, dst
        # (b) the framework route over the views
        if source == "coded":
            views = [dev.motion(b) for b in range(n)]
        else:
            views = [dev.motion_acc(b) for b in range(n)]

        def framework():
            frames = []
            for v in views:
                if source == "coded":
                    has = v[1][..., 0] != 255
                    vec = v[0][:, :, 0, :].float()
                else:
                    has = (v[..., 3] & 0xffff) > 0
                    vec = v[..., :2].clamp(-32768, 32767).float()
                planes = torch.cat([(vec * has[..., None]).permute(2, 0, 1), has[None].float() * 256])
                frames.append(planes.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :h, :w])
            x = torch.nn.functional.interpolate(torch.stack(frames), size=(oh, ow), mode="area")
            return (x * scale).half()
        ref = framework()
        torch.cuda.synchronize()
        # the float route is not the integer definition (area weights, no defined rounding): how far apart they are
        diff = (mine - ref.float()).abs()
        r["framework_max_diff"] = {"vectors_output_px": float(diff[:, :2].max()), "coverage": float(diff[:, 2].max())}
        del ref, diff
        f = timed(framework, 3, args.framework_reps)
        r["framework"] = {"ms": f}
        r["ratio_to_copy"] = c["median"] / t["median"]
        r["ratio_to_framework"] = f["median"] / t["median"]
        res[source] = r
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
    res = {"tool": "motion_scale_bench", "device": v9.device_info(0)[1], "reps": args.reps,
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
