"""GPU parity of intra prediction at frame and tile edges, sample-exact vs the oracle, with the
coverage counted from the packets before anything is launched.

pred_pass (csrc/vp9hip_kernels.hip) fills a job's edges without branches from what the planners
resolved (pl_intra_job: final mode, have_top / have_left, the clamps ct / cl = the last valid
top column / left row, trreal). The clamps do work only where the frame's right or bottom edge
falls inside a transform, which the generator's default draw rarely produces: cut superblocks
mostly split. The frames here (tests/intra_edge_cases.py) are tiny, one whole superblock plus
a cut one or less, drawn with edge_large=1, and every case first asserts, from the walker
(synth_walk.intra_jobs, itself checked against the oracle's trace and the planners on the CPU in
tests/test_intra_edges_host.py), that

  - every final mode occurs at every tx size, luma and chroma, the three DC fills included;
  - every cell (plane class, tx size, final mode, short top / short left edge) that can occur
    does; what cannot is a table with its reasons (intra_edge_cases.NEVER_SHORT, CHROMA32_AVAIL);
  - every clamp length occurs on each edge: luma 16x16 8; luma 32x32 8, 16, 24; 4:2:0 chroma
    8x8 4, 16x16 4, 8, 12;
  - the 4x4 top-right of D45 and D63 is real, replicated without have_right and replicated
    because the frame ends;
  - tile case (520x72, two tile columns): in the second tile's first column (have_left false,
    have_top true) every coded mode occurs at every tx size a block there can have.

Then every executor that predicts intra decodes the frames, every batch twice (the second run
replays the captured graph where there is one): keyframes in batches of 2 (the fused narrow
phase of k_plf) and in one wide batch per size (static plan), by default, under the host
planner (VP9HIP_HOST_PLAN=1) and without the saved SB edge columns (VP9HIP_EDGE=0, the tile
case included); key + P chains whose P frames are mostly intra (p_intra, the census asserted on
the P frames alone) by default (intra workers inside k_lfro), with k_predd as its own launch
(VP9HIP_PRED_LF_FUSE=0), with one k_pred launch per level (VP9HIP_PRED_DF=0) and without k_lfro
(VP9HIP_LFRO=0). 8 bits everywhere; 10 bits on the default keyframe and GOP executors; 12 bits
(base = 128 << 4 in the fills) on one keyframe case; 4:4:4 (32x32 chroma transforms cut by the
edge), 4:2:2 and 4:4:0 keyframes.
"""
import functools
import os

import numpy as np
import pytest

import intra_edge_cases as cases

pytestmark = pytest.mark.gpu

ENVS = {"default": {}, "host": {"VP9HIP_HOST_PLAN": "1"}, "noedge": {"VP9HIP_EDGE": "0"},
        "nofuse": {"VP9HIP_PRED_LF_FUSE": "0"}, "nodf": {"VP9HIP_PRED_DF": "0"}, "nolfro": {"VP9HIP_LFRO": "0"}}


@functools.lru_cache(maxsize=None)
def _covered(v9, kind, fmt):
    """The case's condition, from the packets alone; every test calls it before its first launch."""
    c = cases.census(cases.packets(v9, kind, fmt, inter_only=kind == "gop"))
    if kind == "tile":
        cases.check_tile_census(c)
    else:
        cases.check_census(c, *cases.FORMATS[fmt])
    return True


@pytest.fixture(scope="module")
def devs(v9, gpu):
    """Contexts opened under the environment switches of ENVS (they are read when it opens)."""
    opened = {"default": gpu}

    def get(name):
        if name not in opened:
            env = ENVS[name]
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                opened[name] = v9.Device(0)
            finally:
                for k, x in old.items():
                    if x is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = x
        return opened[name]
    yield get
    for name, d in opened.items():
        if name != "default":
            d.close()


def _cmp(v9, got, ref, w, h, what, ssh, ssv):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


def _run(v9, orc, dev, kind, fmt, bpp, per_batch, what):
    """Decode the case's frames size by size in batches of per_batch frames (0: one batch; whole
    chains in a gop case) and compare every frame with the oracle's."""
    assert _covered(v9, kind, fmt)
    ssh, ssv = cases.FORMATS[fmt]
    refs = cases.references(v9, orc, kind, fmt, bpp)
    for (w, h), fl in cases.frames(v9, kind, fmt, bpp).items():
        n = per_batch or len(fl)
        dev.configure(w, h, bpp, nbufs=n, ss_h=ssh, ss_v=ssv)
        for i0 in range(0, len(fl), n):
            part = fl[i0:i0 + n]
            rb = None
            if kind == "gop":
                rb = [None if r is None else tuple(x - i0 for x in r) for f, r in part]
            dev.stage_batch([f for f, r in part], list(range(len(part))), rb)
            for _ in range(2):
                dev.run_batch()
                dev.sync()
            for k in range(len(part)):
                _cmp(v9, dev.download(k), refs[(w, h)][i0 + k], w, h, "%s %dx%d frame %d" % (what, w, h, i0 + k), ssh, ssv)


KEY_CASES = [("default", "420", 8), ("host", "420", 8), ("noedge", "420", 8), ("default", "420", 10),
             ("default", "444", 8), ("default", "422", 8), ("default", "440", 8)]


@pytest.mark.parametrize("per_batch", [2, 0], ids=["pairs", "wide"])
@pytest.mark.parametrize("env,fmt,bpp", KEY_CASES, ids=["%s-%s-%d" % c for c in KEY_CASES])
def test_keyframes(v9, orc, devs, env, fmt, bpp, per_batch):
    _run(v9, orc, devs(env), "key", fmt, bpp, per_batch, "%s %s %d-bit" % (env, fmt, bpp))


def test_keyframes_12bit(v9, orc, devs):
    _run(v9, orc, devs("default"), "key", "420", 12, 0, "12-bit")


@pytest.mark.parametrize("per_batch", [2, 0], ids=["pairs", "wide"])
@pytest.mark.parametrize("env", ["default", "noedge"])
def test_tile_columns(v9, orc, devs, env, per_batch):
    _run(v9, orc, devs(env), "tile", "420", 8, per_batch, "%s two tile columns" % env)


GOP_CASES = [("default", 8), ("default", 10), ("nofuse", 8), ("nodf", 8), ("nolfro", 8)]


@pytest.mark.parametrize("env,bpp", GOP_CASES, ids=["%s-%d" % c for c in GOP_CASES])
def test_gop_intra_in_p_frames(v9, orc, devs, env, bpp):
    """Chains of a keyframe and 5 P frames, a size's chains in one batch; the P frames' intra
    blocks alone meet the census."""
    _run(v9, orc, devs(env), "gop", "420", bpp, 0, "%s %d-bit GOP" % (env, bpp))
