"""Crafted still pictures for the loop filter (not a test module): pictures whose lines take
every arm of the line routine on non-constant input, sit on each comparison's threshold and one
above it, saturate, and mix arms inside a wavefront; frames whose pre-filter pixels are exactly
such a picture; and the coverage conditions, read from the oracle's census (oracle.LfCensus).
tests/test_lf_cases_host.py checks all of it with the oracle alone, tests/test_gpu_lf_arms.py
runs the frames through every loop-filter kernel.

The frame: an inter frame without intra blocks (p_intra 1e-9) whose coefficients are all set
to 0 with the eobs left as drawn (p_zero_eob 0.5, p_skip 0.5), every motion vector set to 0
with the modes left as drawn (the level's mode index reads mode[3], not the vector), all three
references the same picture: prediction is a copy and every residual is 0, so the loop filter
runs on the uploaded picture. Blocks that keep an eob stay non-skip and filter their inner
transform edges, the rest filter block edges only. (With p_zero_eob 1 the generator, like the
bitstream, vp9block.c:1310-1314, turns every inter block of 8x8 and more without an eob into
a skip block, and no inner transform edge is left above 4x4.) lflvl holds the one level
everywhere.

The picture, per plane, for one (level, sharpness, bit depth) whose E, I, H come from
lf_reference.limits and F = 1 << (bd - 8): 8x8 cells in 32x32 regions that start 8 samples
before each multiple of 32, so that the edges at 0, 8 and 16 modulo 32 lie inside a region.
Region r of a plane takes class (r + seed) modulo the number of classes. Inside a region the
cells' bases alternate like a checkerboard between R and R + d (R random per region), so every
cell edge carries the step d in both directions, and a sample is base + Px[x & 7] + Py[y & 7]
with the class's 8-sample profile P, so a line along either axis shows P plus a constant:

  flat_noise   samples within F of the base at random, step d small: f16 under wd16, f8 under
               wd8, on non-constant lines
  flat_step    constant cells, the same small step
  rough_out    the four samples next to each 16-aligned edge flat, the four beyond them rough:
               f8 under a wd16 edge
  hev          a zigzag of amplitude I (H < amplitude <= I): the hev arm
  n4           a tent (0 0 h a a h 0 0, a = F + 1): nothing next to the edge moves, the line is
               not flat; with the largest step E admits, so that the filter value clamps
  random       every sample random: off
  I_above, H_at, H_above            zigzags of amplitude I + 1, H, H + 1 (hev is I itself)
  Fin_at, Fin_above                 tents of height F and F + 1, small step
  Fout_at, Fout_above               stairs (0 0 0 0 h h a a) of height F and F + 1
  E_at, E_above                     a lip (0 e e e e e e e) on the step d, (d, e) searched so
                                    that 2|p0-q0| + (|p1-q1|>>1) is E, E + 1
  sat_lo, sat_hi                    samples within I of 0 and of 2^bd - 1: both clamps act
  alt_*                             consecutive lines alternate between the flat_step and the
                                    hev or n4 profile, along x or along y: one wavefront holds
                                    lanes of different arms, both ballots see mixed lanes
Chroma planes draw from the arm classes only (no threshold classes: the conditions ask the
tight counters of luma).
"""
import ctypes

import numpy as np

import lf_reference

LEVELS = [(1, 0), (9, 0), (20, 5), (32, 4), (36, 0), (63, 0), (63, 7)]
SIZES = [(200, 136), (66, 130)]
# (level, sharpness, bit depth, ss_h, ss_v)
GROUPS = [(lv, sh, bd, 1, 1) for lv, sh in LEVELS for bd in (8, 10, 12)] + \
         [(36, 0, 8, 0, 0), (36, 0, 8, 1, 0), (36, 0, 8, 0, 1)]
# the first seeds from SEED_BASE on with which every group meets check_group (two frames per
# size and group; bit depth and level do not change what the generator draws)
SEED_BASE = 0xb000
SEEDS = (0xb000, 0xb001)

ARM_CLASSES = ["flat_noise", "flat_step", "rough_out", "hev", "n4", "random", "sat_lo", "sat_hi",
               "alt_hev_x", "alt_hev_y", "alt_n4_x", "alt_n4_y"]
LUMA_CLASSES = ARM_CLASSES + ["I_above", "H_at", "H_above", "Fin_at", "Fin_above", "Fout_at", "Fout_above",
                              "E_at", "E_above"]


def small_step(E, F):
    """The largest of 2F, F, 1 that a constant-sided line passes E's test with."""
    for d in (2 * F, F, 1):
        if 2 * d + (d >> 1) <= E:
            return d
    raise AssertionError("no step passes E = %d" % E)


def e_step(E, I, target):
    """(d, e) with |e| <= I and 2|d + e| + (d >> 1) == target, the smallest |e| first: the lip
    profile (0 e e e e e e e) on a step of d between two cells gives |p0-q0| = |d + e| and
    |p1-q1| = d, with |q1-q0| = |e| the line's only neighbour difference."""
    for e in sorted(range(-I, I + 1), key=abs):
        for d in range(0, target):
            if 2 * abs(d + e) + (d >> 1) == target:
                return d, e
    raise AssertionError("E target %d not met" % target)


def zigzag(a):
    return [0, a, 0, a, 0, a, 0, a]


def tent(a):
    return [0, 0, a // 2, a, a, a // 2, 0, 0]


def stair(a):
    return [0, 0, 0, 0, a // 2, a // 2, a, a]


def class_spec(name, E, I, H, F):
    """(profile of even cells, profile of odd cells, step d, kind): kind None, or 'noise:<n>' (a
    random 0..n per sample, no profile), 'random', 'lo' / 'hi' (noise at the range's end)."""
    z = [0] * 8
    d0 = small_step(E, F)
    big = next(d for d in range(2 * E // 5 + 1, 0, -1) if 2 * d + (d >> 1) <= E)
    rough = [0, 0, 0, 0, 5 * F, 0, 7 * F, 2 * F]
    table = {
        "flat_noise": (z, z, d0, "noise:%d" % F),
        "flat_step": (z, z, d0, None),
        "rough_out": (rough, rough[::-1], d0, None),
        "hev": (zigzag(I), zigzag(I), 0, None),
        "n4": (tent(F + 1), tent(F + 1), big, None),
        "random": (z, z, 0, "random"),
        "sat_lo": (z, z, 0, "lo"),
        "sat_hi": (z, z, 0, "hi"),
        "I_above": (zigzag(I + 1), zigzag(I + 1), 0, None),
        "H_at": (zigzag(H), zigzag(H), 0, None),
        "H_above": (zigzag(H + 1), zigzag(H + 1), 0, None),
        "Fin_at": (tent(F), tent(F), d0, None),
        "Fin_above": (tent(F + 1), tent(F + 1), d0, None),
        "Fout_at": (stair(F), stair(F), 0, None),
        "Fout_above": (stair(F + 1), stair(F + 1), 0, None),
    }
    if name in table:
        return table[name]
    if name in ("E_at", "E_above"):
        d, e = e_step(E, I, E + (name == "E_above"))
        lip = [0] + [e] * 7
        return lip, lip, d, None
    raise KeyError(name)


def class_plane(name, ph, pw, lim, bd, rng):
    """The class's samples relative to its regions' base R (sat_lo / sat_hi: the samples
    themselves), over a whole plane."""
    E, I, H = lim
    F = 1 << (bd - 8)
    pmax = (1 << bd) - 1
    y, x = np.mgrid[0:ph, 0:pw]
    cx, cy = x >> 3, y >> 3
    if name.startswith("alt_"):
        other, axis = name[4:-2], name[-1]
        a = class_plane("flat_step", ph, pw, lim, bd, rng)
        pe, po, _, _ = class_spec(other, E, I, H, F)
        d = small_step(E, F)
        along, line = (x, y) if axis == "x" else (y, x)
        b = np.asarray(pe)[along & 7] + ((cx + cy) & 1) * d
        return np.where(line & 1, b, a)
    pe, po, d, kind = class_spec(name, E, I, H, F)
    if kind == "random":
        return rng.integers(-(pmax // 4), pmax // 4 + 1, (ph, pw))
    if kind in ("lo", "hi"):
        n = rng.integers(0, I + 1, (ph, pw))                        # absolute, not relative to R
        return n if kind == "lo" else pmax - n
    if kind:
        return rng.integers(0, int(kind[6:]) + 1, (ph, pw)) + ((cx + cy) & 1) * d
    P = np.asarray([pe, po])
    return P[cx & 1, x & 7] + P[cy & 1, y & 7] + ((cx + cy) & 1) * d


def plane_picture(ph, pw, lim, bd, seed, classes):
    """One plane of ph x pw samples (multiples of 8) as int64, every sample in range."""
    E, I, H = lim
    pmax = (1 << bd) - 1
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ph, 0:pw]
    nrx = (pw + 8 + 31) >> 5
    nry = (ph + 8 + 31) >> 5
    region = ((y + 8) >> 5) * nrx + ((x + 8) >> 5)
    cls = (np.arange(nrx * nry) + seed) % len(classes)
    base = rng.integers(pmax // 4, 3 * pmax // 4, nrx * nry)
    out = np.zeros((ph, pw), np.int64)
    for k, name in enumerate(classes):
        t = class_plane(name, ph, pw, lim, bd, rng)
        out = np.where(cls[region] == k, t if name in ("sat_lo", "sat_hi") else base[region] + t, out)
    return np.clip(out, 0, pmax)


def picture(v9, w, h, bd, level, sharp, seed, ssh=1, ssv=1):
    """The three padded planes (v9.alloc_planes layout) for a frame of w x h."""
    lim = lf_reference.limits(level, sharp, bd)
    planes = v9.alloc_planes(w, h, bd, ssh, ssv)
    for p, a in enumerate(planes):
        a[:] = plane_picture(a.shape[0], a.shape[1], lim, bd, seed * 3 + p, LUMA_CLASSES if p == 0 else ARM_CLASSES)
    return planes


def frame(v9, w, h, bd, level, sharp, seed, ssh=1, ssv=1):
    """The inter frame that copies its references and filters them at the one level."""
    f = v9.SynthFrame(v9.synth_params(w, h, bd, seed=seed, inter=1, p_intra=1e-9, p_zero_eob=0.5, p_skip=0.5,
                                      filter_level=level, sharpness=sharp, ss_h=ssh, ss_v=ssv))
    for b in f.blocks():
        for k in range(16):
            b.mv[k] = 0
    ctypes.memset(f.pkt.coefs, 0, f.nbytes_coefs)
    for k in range(64):
        f.pkt.lflvl[k] = level
    return f


def group_frames(v9, group):
    """[(frame, picture)] of a group: SEEDS at each of SIZES."""
    level, sharp, bd, ssh, ssv = group
    return [(frame(v9, w, h, bd, level, sharp, seed, ssh, ssv), picture(v9, w, h, bd, level, sharp, seed, ssh, ssv))
            for w, h in SIZES for seed in SEEDS]


def oracle_census(v9, orc, f, pic):
    """(the oracle's output planes, the census of its loop filter) of one crafted frame."""
    out = v9.alloc_planes(f.pkt.width, f.pkt.height, f.pkt.bpp, f.pkt.ss_h, f.pkt.ss_v)
    with orc.LfCensus() as c:
        orc.decode_frame(f.pkt, out, [pic, pic, pic])
    return out, c


def unreachable(group):
    """The census cells no picture can fill in this group, each with its derivation:
    [(plane class, arm name, why)]; they hold for both directions and all widths."""
    level, sharp, bd, ssh, ssv = group
    E, I, H = lf_reference.limits(level, sharp, bd)
    out = []
    if I <= H:
        why = "a filtered line has |p1-p0| <= I and |q1-q0| <= I, hev needs one of them > H, and I = %d <= H = %d" % (I, H)
        out += [(0, "h4", why), (1, "h4", why)]
    # chroma f16: a wd16 chroma edge needs a chroma transform of 16x16 or more (mask_edges,
    # vp9block.c:1213-1250), whose block covers 16 << ss chroma-subsampled luma samples; every
    # size of SIZES holds one in every layout, so no group lists it
    if any(min((w + 7) & ~7, (h + 7) & ~7) < 16 << max(ssh, ssv) for w, h in SIZES):
        out.append((1, "f16", "no block of these frames can carry a 16x16 chroma transform"))
    return out


def tight_representable(group):
    """Per oracle.LF_TIGHT counter, whether a line can hold it: a line that reaches the 4-wide
    arms has |p1-p0| <= I, so H's counters need H <= I (at) and H + 1 <= I (above); the others
    always can (I, E: the mask's own inputs; F, F + 1 <= 2 I are reached in two steps of <= I)."""
    level, sharp, bd, ssh, ssv = group
    E, I, H = lf_reference.limits(level, sharp, bd)
    return [True] * 8 + [H <= I, H + 1 <= I]


def check_group(orc, group, censuses, need=8):
    """The coverage conditions of a group over its frames' censuses; raises AssertionError with
    every miss. Returns (count, moved, tight) summed."""
    count = sum(c.count for c in censuses)
    moved = sum(c.moved for c in censuses)
    tight = sum(c.tight for c in censuses)
    skip = {(p, a) for p, a, _ in unreachable(group)}
    miss = []
    for p in range(2):
        for d in range(2):
            for a, arm in enumerate(orc.LF_ARMS):
                if (p, arm) in skip:
                    assert count[p, d, :, a].sum() == 0, "unreachable cell %s has lines" % ((p, d, arm),)
                    continue
                n = (count if arm == "off" else moved)[p, d, :, a].sum()
                if n < need:
                    miss.append("plane class %d dir %d %s: %d" % (p, d, arm, n))
    for d in range(2):
        for a, what in ((3, "f8 under wd16"), (4, "f16")):
            if moved[0, d, 2, a] < need:
                miss.append("luma dir %d %s: %d" % (d, what, moved[0, d, 2, a]))
    for k, ok in enumerate(tight_representable(group)):
        if ok and tight[0, k] < need:
            miss.append("luma tight %s: %d" % (orc.LF_TIGHT[k], tight[0, k]))
    assert not miss, "group %s: %s" % (group, "; ".join(miss))
    return count, moved, tight


# ---- every level and sharpness in natural frames -------------------------------------------
NATURAL_SIZE = (200, 136)
NATURAL_SEED = 0xb100
ZEROMV = 12                                                  # VP9H_ZEROMV (include/vp9hip.h)
SEG8 = {"enabled": 1, "update_map": 1, "update_data": 1, "nseg": 8}


def block_level(pkt, b):
    """The level the frame path gives a block (vp9block.c:1438): lflvl[seg][ref row][mode]."""
    return pkt.lflvl[b.seg_id * 8 + (0 if b.intra else b.ref[0] + 1) * 2 + (b.mode[3] != ZEROMV)]


def natural_set(v9, bd):
    """[(frame, is_key)], 24 frames of default generator content with 8 segments: per sharpness
    0..7 two inter frames (compound, every reference) whose 48 lflvl entries (8 segments x 3
    references x 2 modes) hold 48 distinct levels, 0..47 in the first and 16..63 in the second,
    rotated by the sharpness, and one keyframe with 8 distinct levels, sharpness + 8 * segment.
    An inter frame's intra row holds 63 - 8 * segment."""
    w, h = NATURAL_SIZE
    out = []
    for sharp in range(8):
        for i in range(2):
            f = v9.SynthFrame(v9.synth_params(w, h, bd, seed=NATURAL_SEED + 4 * sharp + i, inter=1, compound=1, ref_mix=1,
                                              seg=SEG8, sharpness=sharp, filter_level=32))
            for s in range(8):
                f.pkt.lflvl[s * 8] = f.pkt.lflvl[s * 8 + 1] = 63 - 8 * s
                for k in range(6):
                    f.pkt.lflvl[s * 8 + 2 + k] = 16 * i + (s * 6 + k + 5 * sharp) % 48
            out.append((f, False))
        f = v9.SynthFrame(v9.synth_params(w, h, bd, seed=NATURAL_SEED + 4 * sharp + 2, seg=SEG8, sharpness=sharp,
                                          filter_level=32))
        for s in range(8):
            for k in range(8):
                f.pkt.lflvl[s * 8 + k] = sharp + 8 * s
        out.append((f, True))
    return out


def check_natural_levels(frames, need=4):
    """Every level 0..63 is the level of at least `need` blocks across the set."""
    used = [0] * 64
    for f, _ in frames:
        for b in f.blocks():
            used[block_level(f.pkt, b)] += 1
    assert min(used) >= need, "blocks per level: %s" % used
    return used


_CACHE = {}


def group_oracle(v9, orc, group):
    """[(frame, picture, oracle output, census)] of a crafted group, computed once a session."""
    if group not in _CACHE:
        _CACHE[group] = [(f, pic) + oracle_census(v9, orc, f, pic) for f, pic in group_frames(v9, group)]
    return _CACHE[group]


def natural_oracle(v9, orc, bd):
    """(the three reference pictures, [(frame, is_key, oracle output, census)]) of natural_set;
    the references are the oracle's outputs of three keyframes, computed once a session."""
    if ("natural", bd) not in _CACHE:
        w, h = NATURAL_SIZE
        keys = []
        for i in range(3):
            k = v9.alloc_planes(w, h, bd)
            key = v9.SynthFrame(v9.synth_params(w, h, bd, seed=NATURAL_SEED + 0x80 + i))   # owns the packet's arrays
            orc.decode_frame(key.pkt, k)
            keys.append(k)
        res = []
        for f, is_key in natural_set(v9, bd):
            out = v9.alloc_planes(w, h, bd)
            with orc.LfCensus() as c:
                orc.decode_frame(f.pkt, out, None if is_key else keys)
            res.append((f, is_key, out, c))
        _CACHE[("natural", bd)] = (keys, res)
    return _CACHE[("natural", bd)]


def tight_line(cmp, above, lim, bd):
    """For test_lf_reference: (16-sample line, coded width, expected arm) with comparison
    cmp ('I', 'E', 'Fin', 'Fout', 'H') at its threshold, or one above it; None where
    tight_representable says no line can."""
    E, I, H = lim
    F = 1 << (bd - 8)
    b = 1 << (bd - 1)
    t = [b] * 16
    if cmp == "I":
        t[11] = b + I + above                                # q3 alone
        return t, 4, "off" if above else "n4"
    if cmp == "E":
        d, e = e_step(E, I, E + above)
        t[:8] = [b + d + e] * 8                              # p side constant
        t[8] = b                                             # q0
        t[9:] = [b + e] * 7                                  # q1 ..: |p1-q1| = d, |p0-q0| = d + e
        return t, 4, "off" if above else "h4" if abs(e) > H else "n4"
    if cmp == "Fin":
        a = F + above
        t[10], t[11] = b + a // 2, b + a
        return t, 8, "n4" if above else "f8"
    if cmp == "Fout":
        t[15] = b + F + above
        return t, 16, "f8" if above else "f16"
    if cmp == "H":
        a = H + above
        if a > I:
            return None
        t[6] = b + a                                         # p1
        t[5] = t[4] = b + a
        return t, 4, "h4" if above else "n4"
    raise KeyError(cmp)
