"""Every arm of the loop filter's line routine (lf_reg) through every loop-filter kernel,
sample-exact against the oracle, with the arms counted by the oracle's census.

Whole-frame parity on the generator's default content leaves the 15-tap arm on constant lines
only (its fixed point) and puts no comparison on its threshold. Here:

  crafted  the still pictures of tests/lf_cases.py (every arm on lines that move, the 7-tap
           arm under a 16-wide edge, each of the five comparisons on its threshold and one
           above, both clamps, wavefronts whose lanes take different arms) as the pre-filter
           pixels of inter frames, at seven (level, sharpness) pairs, 8 / 10 / 12 bits, two
           sizes with partial superblocks on both axes, 4:2:0 and one group each of 4:4:4,
           4:2:2 and 4:4:0. The coverage conditions are asserted from the oracle before the
           device runs (tests/test_lf_cases_host.py asserts them on the CPU). Each group runs
           on three fresh contexts: the default (narrow phases take k_lfr and so k_lfro),
           VP9HIP_LFRO=0 (k_lfrd) and VP9HIP_LFROW=0 (the diagonal k_lf, whose first steps
           are k_plf launches); a timed run, whose launch classes are asserted, then two
           runs of the captured graph.
  natural  default generator content with 8 segments whose lflvl tables are overwritten so
           that 24 frames (two compound inter frames and a keyframe per sharpness 0..7) use
           every level 0..63, level 0 included (its edges stay unfiltered); in batches of at
           most 4 frames of one kind (narrow phases: k_lfr, with k_plf for keyframes) and as one
           batch of 24 (phases of 8 frames and more: the diagonal kernels with per-frame
           sharpness in one launch).
"""
import numpy as np
import pytest

import lf_cases

pytestmark = pytest.mark.gpu

# (id, environment, the timing classes that must have launches, those that must have none)
KERNELS = [("k_lfro", {}, ("k_lfr",), ("k_lf", "k_plf")),
           ("k_lfrd", {"VP9HIP_LFRO": "0"}, ("k_lfr",), ("k_lf", "k_plf")),
           ("k_lf", {"VP9HIP_LFROW": "0"}, ("k_lf",), ("k_lfr",))]


def _cmp(v9, got, ref, w, h, what, ssh=1, ssv=1):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


def _launches(dev, with_launches, without):
    """The last timed run's launch counts per class: some in each of with_launches, none in
    the classes of without."""
    t = {k: v[1] for k, v in dev.timing().items()}
    assert all(t[k] > 0 for k in with_launches) and all(t[k] == 0 for k in without), t
    return t


def _gid(g):
    return "L%d_S%d_%dbit_ss%d%d" % g


@pytest.mark.parametrize("group", lf_cases.GROUPS, ids=_gid)
def test_crafted_pictures_through_every_kernel(v9, orc, monkeypatch, group):
    bd, ssh, ssv = group[2:]
    res = lf_cases.group_oracle(v9, orc, group)
    lf_cases.check_group(orc, group, [c for _, _, _, c in res])
    for kid, env, on, off in KERNELS:
        with monkeypatch.context() as m:
            for k, val in env.items():
                m.setenv(k, val)                             # read when the context opens
            dev = v9.Device(0)
        try:
            for w, h in lf_cases.SIZES:
                batch = [r for r in res if (r[0].pkt.width, r[0].pkt.height) == (w, h)]
                n = len(batch)
                dev.configure(w, h, bd, nbufs=2 * n, ss_h=ssh, ss_v=ssv)
                for i, (f, pic, out, c) in enumerate(batch):
                    dev.upload(i, pic)
                dev.stage_batch([f for f, _, _, _ in batch], [n + i for i in range(n)], [(i, i, i) for i in range(n)])
                for run in range(3):
                    dev.set_timing(run == 0)                 # then twice the captured graph
                    dev.run_batch()
                    dev.sync()
                    if run == 0:
                        print(kid, _gid(group), "%dx%d:" % (w, h), _launches(dev, on, off))
                    if run != 1:
                        for i, (f, pic, out, c) in enumerate(batch):
                            _cmp(v9, dev.download(n + i), out, w, h,
                                 "%s %s %dx%d frame %d run %d" % (kid, _gid(group), w, h, i, run), ssh, ssv)
        finally:
            dev.close()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("one_batch", [0, 1], ids=["batches_of_4", "one_batch"])
def test_every_level_and_sharpness(v9, orc, gpu, one_batch, bd):
    w, h = lf_cases.NATURAL_SIZE
    keys, res = lf_cases.natural_oracle(v9, orc, bd)
    lf_cases.check_natural_levels([(f, k) for f, k, _, _ in res])
    assert all(c.moved.sum() > 0 for _, _, _, c in res)
    inter = [r for r in res if not r[1]]
    key = [r for r in res if r[1]]
    if one_batch:
        batches = [(res, ("k_lf", "k_plf"), ("k_lfr",))]
    else:
        batches = [(inter[i:i + 4], ("k_lfr",), ("k_lf", "k_plf")) for i in range(0, len(inter), 4)] + \
                  [(key[i:i + 4], ("k_lfr", "k_plf"), ("k_lf",)) for i in range(0, len(key), 4)]
    gpu.configure(w, h, bd, nbufs=3 + len(res))
    for i in range(3):
        gpu.upload(i, keys[i])
    try:
        for bi, (batch, on, off) in enumerate(batches):
            n = len(batch)
            gpu.stage_batch([r[0] for r in batch], [3 + i for i in range(n)], [None if r[1] else (0, 1, 2) for r in batch])
            for run in range(2):
                gpu.set_timing(run == 0)
                gpu.run_batch()
                gpu.sync()
                if run == 0:
                    print("natural %d-bit batch %d:" % (bd, bi), _launches(gpu, on, off))
            for i, (f, is_key, out, c) in enumerate(batch):
                _cmp(v9, gpu.download(3 + i), out, w, h, "%d-bit batch %d frame %d (sharpness %d, %s)"
                     % (bd, bi, i, f.pkt.sharpness, "key" if is_key else "inter"))
    finally:
        gpu.set_timing(True)
