"""The oracle's loop-filter line routine and limit tables against an independent statement of
the VP9 specification's text (tests/lf_reference.py, plain Python integers), exactly (CPU).

The oracle and the kernels were written from one reading of vp9dsp_template.c; the property
tests of test_oracle_dsp.py would pass a shared misreading. Here every entry point of
orc.loop_filter (8 lines at width 4 and 8, 16 lines at width 16, mix2 with the four width pairs
and two different (E, I, H)), both directions, 8 / 10 / 12 bits, over random lines, lines of
every class lf_cases crafts, saturated lines and lines that put each of the five comparisons on
its threshold and one above it, with the arm each line takes read from the oracle's census
(vp9o_set_lf_census) and compared with the reference's."""
import collections

import numpy as np
import pytest

import lf_cases
import lf_reference

KINDS = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1)]
WIDTH = {4: 0, 8: 1, 16: 2}


def test_limit_tables(orc):
    for level in range(64):
        for sharp in range(8):
            assert orc.lf_limits(level, sharp) == lf_reference.limits(level, sharp), (level, sharp)


def _lines(level, sharp, bd, seed):
    """(n, 16) lines for one level: random of three kinds, the crafted classes, the range's ends."""
    E, I, H = lim = lf_reference.limits(level, sharp, bd)
    F, pmax = 1 << (bd - 8), (1 << bd) - 1
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, pmax + 1, (16, 16))]
    walk = np.cumsum(rng.integers(-I - 1, I + 2, (48, 16)), axis=1) + rng.integers(pmax // 4, pmax // 2, (48, 1))
    out.append(walk)
    flat = rng.integers(0, F + 2, (48, 16)) + rng.integers(pmax // 4, pmax // 2, (48, 1))
    flat[:, 8:] += rng.integers(-E // 2 - 1, E // 2 + 2, (48, 1))
    out.append(flat)
    for end in (0, pmax):                                   # both clamps
        out.append(np.abs(end - rng.integers(0, 2 * I + 2, (24, 16))))
        out.append(np.abs(end - np.abs(np.cumsum(rng.integers(-I, I + 1, (24, 16)), axis=1))))
    for k, name in enumerate(lf_cases.LUMA_CLASSES):
        pic = lf_cases.plane_picture(32, 48, lim, bd, seed + k, [name])
        out += [pic[8:16, 8:24], pic[16:24, 16:32], pic[8:24, 12:28][::2], pic[8:24, 8:24].T[4:12]]
    return np.clip(np.concatenate(out), 0, pmax)


@pytest.mark.parametrize("direction", [0, 1], ids=["cols", "rows"])
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("kind,wd1,wd2", KINDS, ids=["lf8_4", "lf8_8", "lf16", "mix44", "mix48", "mix84", "mix88"])
def test_line_routine_equals_the_specification(orc, kind, wd1, wd2, bd, direction):
    dt = np.uint8 if bd == 8 else np.uint16
    n_lines = 0
    for li, (level, sharp) in enumerate(lf_cases.LEVELS):
        lines = _lines(level, sharp, bd, 1000 * bd + 10 * li + direction)
        lines = lines[:len(lines) // 16 * 16]
        n_lines += len(lines)
        img = np.ascontiguousarray((lines if direction == 0 else lines.T).astype(dt))
        ref = img.astype(np.int64)
        E, I, H = lf_reference.limits(level, sharp)
        if kind == 2:                                       # the second eight lines at another level
            E2, I2, H2 = lf_reference.limits(*lf_cases.LEVELS[(li + 3) % len(lf_cases.LEVELS)])
            assert (E2, I2, H2) != (E, I, H)
            E, I, H = E | E2 << 8, I | I2 << 8, H | H2 << 8
        per_call = 8 if kind == 0 else 16
        arms = []
        with orc.LfCensus() as census:
            for k in range(0, len(lines), per_call):
                y, x = (k, 8) if direction == 0 else (8, k)
                orc.loop_filter(bd, img, y * img.shape[1] + x, img.shape[1], kind, wd1, wd2, direction, E, I, H)
                arms += lf_reference.apply(ref, y, x, kind, wd1, wd2, direction, E, I, H, bd)
        assert np.array_equal(img, ref), "level %d sharpness %d: %d samples differ" % (level, sharp, (img != ref).sum())
        # the census saw the same lines take the same arms (luma, this direction, any width)
        seen = collections.Counter(arms)
        assert [seen[a] for a in lf_reference.ARMS] == list(census.count[0, direction].sum(axis=0)), (level, sharp)
        assert census.count.sum() == len(lines)
        widest = 16 if kind == 1 else 4 << max(wd1, wd2 if kind == 2 else 0)
        for a in ("off", "n4") + (("h4",) if I & 0xff > H & 0xff else ()) + (("f8",) if widest >= 8 else ()) + \
                (("f16",) if widest == 16 else ()):
            assert seen[a] >= 16, "level %d sharpness %d: %d %s lines" % (level, sharp, seen[a], a)
    assert n_lines >= 2000


@pytest.mark.parametrize("direction", [0, 1], ids=["cols", "rows"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_each_comparison_at_its_threshold(orc, bd, direction):
    """Eight copies of a line with one comparison at its threshold, then one above it: the census
    holds them in the expected arm's cell and in the comparison's tight counter, the reference
    takes the same arm and gives the same samples."""
    dt = np.uint8 if bd == 8 else np.uint16
    for level, sharp in lf_cases.LEVELS:
        lim = lf_reference.limits(level, sharp, bd)
        can = lf_cases.tight_representable((level, sharp, bd, 1, 1))
        for ci, cmp in enumerate(("I", "E", "Fin", "Fout", "H")):
            for above in (0, 1):
                made = lf_cases.tight_line(cmp, above, lim, bd)
                assert (made is not None) == can[2 * ci + above], (level, sharp, cmp, above)
                if made is None:
                    continue
                line, wd, arm = made
                lines = np.tile(np.asarray(line), (8, 1))
                img = np.ascontiguousarray((lines if direction == 0 else lines.T).astype(dt))
                ref = img.astype(np.int64)
                y, x = (0, 8) if direction == 0 else (8, 0)
                E, I, H = lf_reference.limits(level, sharp)
                with orc.LfCensus() as census:
                    orc.loop_filter(bd, img, y * img.shape[1] + x, img.shape[1], 0, WIDTH[wd], 0, direction, E, I, H)
                arms = lf_reference.apply(ref, y, x, 0, WIDTH[wd], 0, direction, E, I, H, bd)
                what = "level %d sharpness %d %s%s" % (level, sharp, cmp, "+1" if above else "")
                assert arms == [arm] * 8, what
                assert census.count[0, direction, WIDTH[wd], lf_reference.ARMS.index(arm)] == 8, what
                assert census.tight[0, 2 * ci + above] == 8, what
                assert np.array_equal(img, ref), what
