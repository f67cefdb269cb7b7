"""The VP9 loop filter's line routine and limits in plain Python integers, written from the
specification's form (VP9 bitstream specification, sections 8.8.1 and 8.8.2), not from the
oracle (oracle/vp9o_dsp_tmpl.h) or the kernel (lf_reg): the third statement the other two are
checked against (tests/test_lf_reference.py).

A line is the 16 samples across an edge, T[-8] .. T[7]: T[i] = q_i for i >= 0 and p_(-i-1)
for i < 0, held here as a list t with t[8 + i] = T[i].
"""

ARMS = ("off", "n4", "h4", "f8", "f16")


def clip3(lo, hi, x):
    return lo if x < lo else hi if x > hi else x


def round2(x, n):
    return (x + (1 << (n - 1))) >> n


def limits(level, sharp, bd=8):
    """(blimit, limit, thresh) of a filter level: 8.8.1, shifted to the bit depth."""
    shift = 2 if sharp > 4 else 1 if sharp > 0 else 0
    limit = clip3(1, 9 - sharp, level >> shift) if sharp > 0 else max(1, level >> shift)
    blimit = 2 * (level + 2) + limit
    thresh = level >> 4
    return blimit << (bd - 8), limit << (bd - 8), thresh << (bd - 8)


def masks(t, blimit, limit, thresh, bd):
    """(hevMask, filterMask, flatMask, flatMask2) of a line: 8.8.2's filter mask process."""
    T = lambda i: t[8 + i]
    one = 1 << (bd - 8)
    hev = abs(T(-2) - T(-1)) > thresh or abs(T(1) - T(0)) > thresh
    fm = all(abs(T(-i - 2) - T(-i - 1)) <= limit and abs(T(i + 1) - T(i)) <= limit for i in range(3)) \
        and abs(T(-1) - T(0)) * 2 + abs(T(-2) - T(1)) // 2 <= blimit
    flat = all(abs(T(-i - 1) - T(-1)) <= one and abs(T(i) - T(0)) <= one for i in range(1, 4))
    flat2 = all(abs(T(-i - 1) - T(-1)) <= one and abs(T(i) - T(0)) <= one for i in range(4, 8))
    return hev, fm, flat, flat2


def narrow(t, hev, bd):
    """The narrow filter process: p1 .. q1 of a copy of t."""
    o = list(t)
    half = 0x80 << (bd - 8)
    c4 = lambda x: clip3(-(1 << (bd - 1)), (1 << (bd - 1)) - 1, x)
    ps1, ps0, qs0, qs1 = t[6] - half, t[7] - half, t[8] - half, t[9] - half
    f = c4(ps1 - qs1) if hev else 0
    f = c4(f + 3 * (qs0 - ps0))
    filter1 = c4(f + 4) >> 3
    filter2 = c4(f + 3) >> 3
    o[8] = c4(qs0 - filter1) + half
    o[7] = c4(ps0 + filter2) + half
    if not hev:
        f = round2(filter1, 1)
        o[9] = c4(qs1 - f) + half
        o[6] = c4(ps1 + f) + half
    return o


def wide(t, n):
    """The wide filter process with n = 3 (log2Size 3) or n = 7 (log2Size 4): F[-n] .. F[n - 1]."""
    o = list(t)
    log2size = 3 if n == 3 else 4
    for i in range(-n, n):
        acc = 0
        for j in range(-n, n + 1):
            tap = 2 if j == 0 else 1
            acc += tap * t[8 + clip3(-(n + 1), n, i + j)]
        o[8 + i] = round2(acc, log2size)
    return o


def filter_line(t, wd, blimit, limit, thresh, bd):
    """A 16-sample line filtered at coded width wd (4, 8, 16) with limits already shifted to the
    bit depth: (the new line or None, the arm's name). Width 4 and 8 change p3 .. q3 at most."""
    hev, fm, flat, flat2 = masks(t, blimit, limit, thresh, bd)
    if not fm:
        return None, "off"
    if wd >= 16 and flat and flat2:
        return wide(t, 7), "f16"
    if wd >= 8 and flat:
        return wide(t, 3), "f8"
    return narrow(t, hev, bd), "h4" if hev else "n4"


def apply(img, y, x, kind, wd1, wd2, direction, E, I, H, bd):
    """orc.loop_filter's call on a 2-D array of Python-int-convertible samples, in place: the
    edge lies before sample (y, x); kind 0: 8 lines at width 4 << wd1, 1: 16 lines at width 16,
    2 (mix2): 8 lines at 4 << wd1 with the low bytes of E, I, H, then 8 at 4 << wd2 with the
    bytes above; direction 0: a column edge (lines along x, one per row), 1: a row edge. E, I, H
    before the bit-depth shift. Returns the arms of the lines."""
    runs = {0: [(4 << wd1, E, I, H)], 1: [(16, E, I, H)] * 2,
            2: [(4 << wd1, E & 0xff, I & 0xff, H & 0xff), (4 << wd2, E >> 8, I >> 8, H >> 8)]}[kind]
    arms = []
    for r, (wd, e, i, h) in enumerate(runs):
        s = bd - 8
        for k in range(8):
            n = 8 * r + k
            yy, xx = (y + n, x) if direction == 0 else (y, x + n)
            half = 8 if wd == 16 else 4
            idx = [(yy, xx + d) if direction == 0 else (yy + d, xx) for d in range(-half, half)]
            t = [0] * 16
            for d, (a, b) in zip(range(-half, half), idx):
                t[8 + d] = int(img[a, b])
            o, arm = filter_line(t, wd, e << s, i << s, h << s, bd)
            arms.append(arm)
            if o is not None:
                for d, (a, b) in zip(range(-half, half), idx):
                    img[a, b] = o[8 + d]
    return arms
