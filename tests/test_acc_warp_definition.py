"""Accumulated residual: a numpy restatement of the definition in include/vp9hip.h ("accumulated
residual"), sharing no code with the library, against vp9hip_acc_warp_host (CPU suite).

warp_ref / warp_stats / hand_cases below are what tests/test_gpu_acc_warp.py compares the kernel
with. Hand-made fields on a 6 x 4 grid (24 x 16 luma) pin every bilinear phase, the rounding of
negative vectors, the clamp of the sums to int16, the clamps at the four plane edges, the rule
that decides whether a cell applies, both outputs, the int16 clamp of the residual and the mask;
planes 1 sample wide, odd planes and pitched planes with poison beyond the visible width pin the
bounds. All comparisons are exact.

Phases: a luma vector is in 1/8 sample and is doubled to 1/16, so luma phases (fx, fy) are even
by definition: the 64 even pairs are all a luma plane can show, and each is covered. Chroma at
4:2:0 takes the vector as it is and shows all 256 pairs, each covered; 4:4:4 chroma behaves as
luma.
"""
import re

import numpy as np
import pytest

from test_motion_acc_definition import CELL, INTRA, NOFIELD, SCALED

I32MAX, I32MIN = 2 ** 31 - 1, -2 ** 31


def _geometry(w, h, sh, sv, p):
    s_h, s_v = (sh, sv) if p else (0, 0)
    return s_h, s_v, (w + s_h) >> s_h, (h + s_v) >> s_v


def warp_ref(A, B, acc, sb, w, h, sh, sv, interp, output):
    """The definition for one pair: A, B three 2-D planes each (at least the visible size), acc a
    CELL array (GH, GW), sb the serial of b. Returns ([y, u, v] int16, mask uint8 (GH, GW))."""
    app = (acc["hops"] > 0) & (acc["root"] == np.uint32(sb))
    vx = np.clip(acc["dx"].astype(np.int64), -32768, 32767)
    vy = np.clip(acc["dy"].astype(np.int64), -32768, 32767)
    out = []
    for p in range(3):
        s_h, s_v, pw, ph = _geometry(w, h, sh, sv, p)
        ys, xs = np.mgrid[0:ph, 0:pw].astype(np.int64)
        r, c = (ys << s_v) >> 2, (xs << s_h) >> 2
        ap, Px, Py = app[r, c], vx[r, c] * (2 >> s_h), vy[r, c] * (2 >> s_v)
        a, b = np.asarray(A[p])[:ph, :pw].astype(np.int64), np.asarray(B[p])[:ph, :pw].astype(np.int64)
        cx, cy = (lambda v: np.clip(v, 0, pw - 1)), (lambda v: np.clip(v, 0, ph - 1))
        if interp == "nearest":
            pred = b[cy(ys + ((Py + 8) >> 4)), cx(xs + ((Px + 8) >> 4))]       # numpy's >> floors
        else:
            x0, y0, fx, fy = xs + (Px >> 4), ys + (Py >> 4), Px & 15, Py & 15
            pred = ((16 - fx) * (16 - fy) * b[cy(y0), cx(x0)] + fx * (16 - fy) * b[cy(y0), cx(x0 + 1)] +
                    (16 - fx) * fy * b[cy(y0 + 1), cx(x0)] + fx * fy * b[cy(y0 + 1), cx(x0 + 1)] + 128) >> 8
        if output == "residual":
            out.append(np.where(ap, np.clip(a - pred, -32768, 32767), 0).astype(np.int16))
        else:
            out.append(np.where(ap, pred, a).astype(np.uint16).view(np.int16))
    return out, app.astype(np.uint8)


def warp_stats(acc, sb, w, h, sh=1, sv=1):
    """What a pair exercises, from the reference alone: applying cells over cells, of the applying
    cells with a visible luma sample the share with one whose nearest-mode source is clamped at a
    plane edge, the
    four sides (left, right, top, bottom) at which any plane clamps, and the (fx, fy) phases of
    applying samples of luma and of chroma."""
    app = (acc["hops"] > 0) & (acc["root"] == np.uint32(sb))
    vx = np.clip(acc["dx"].astype(np.int64), -32768, 32767)
    vy = np.clip(acc["dy"].astype(np.int64), -32768, 32767)
    sides, phases, edge_cells, seen = np.zeros(4, bool), [set(), set()], np.zeros(acc.shape, bool), np.zeros(acc.shape, bool)
    for p in range(2):
        s_h, s_v, pw, ph = _geometry(w, h, sh, sv, p)
        ys, xs = np.mgrid[0:ph, 0:pw].astype(np.int64)
        r, c = (ys << s_v) >> 2, (xs << s_h) >> 2
        ap, Px, Py = app[r, c], vx[r, c] * (2 >> s_h), vy[r, c] * (2 >> s_v)
        tx, ty = xs + ((Px + 8) >> 4), ys + ((Py + 8) >> 4)
        hit = [ap & (tx < 0), ap & (tx > pw - 1), ap & (ty < 0), ap & (ty > ph - 1)]
        sides |= np.array([m.any() for m in hit])
        if p == 0:
            np.logical_or.at(edge_cells, (r, c), hit[0] | hit[1] | hit[2] | hit[3])
            np.logical_or.at(seen, (r, c), ap)
        phases[p] = set(zip((Px & 15)[ap].tolist(), (Py & 15)[ap].tolist()))
    napp, nseen = int(app.sum()), int(seen.sum())
    return dict(applying=napp / app.size, edge=(int(edge_cells.sum()) / nseen if nseen else 0.0), sides=sides,
                luma_phases=phases[0], chroma_phases=phases[1])


GW, GH, W, H = 6, 4, 24, 16


def _planes(rng, w, h, bpp, sh, sv, pad=0, poison=None, top=None):
    """Random planes of exactly the visible size, as views of arrays `pad` samples wider that hold
    `poison` beyond the width."""
    dt = np.uint8 if bpp == 8 else np.uint16
    out = []
    for p in range(3):
        _, _, pw, ph = _geometry(w, h, sh, sv, p)
        full = np.full((ph, pw + pad), (1 << bpp) - 1 if poison is None else poison, dt)
        full[:, :pw] = rng.integers(0, top if top is not None else 1 << bpp, (ph, pw))
        out.append(full[:, :pw])
    return out


def _acc(gw, gh, dx, dy, root, hops=1, end=INTRA):
    a = np.zeros((gh, gw), CELL)
    a["dx"], a["dy"], a["root"], a["hops"], a["end"] = dx, dy, root, hops, end
    return a


def hand_cases():
    """(name, A, B, acc, sb, w, h, bpp, sh, sv): the hand-made pairs."""
    rng = np.random.default_rng(1803)
    cells = np.arange(GW * GH).reshape(GH, GW)
    for sh, sv, bpp in ((1, 1, 8), (0, 0, 8), (1, 1, 10), (0, 0, 10)):
        tag = "%s-%dbit" % ("420" if sh else "444", bpp)
        # every phase: cell i of field k has (fx, fy) = the two nibbles of 24 k + i, and a whole part of -3 .. 3
        for k in range(11):
            idx = (24 * k + cells) % 256
            dx = 16 * ((cells + k) % 7 - 3) + (idx & 15)
            dy = 16 * ((cells * 3 + k) % 7 - 3) + (idx >> 4)
            yield ("phases%d-%s" % (k, tag), _planes(rng, W, H, bpp, sh, sv), _planes(rng, W, H, bpp, sh, sv),
                   _acc(GW, GH, dx, dy, 5, hops=1 + k), 5, W, H, bpp, sh, sv)
        # the named vectors, every pairing of a row of them with a shifted row
        V = np.array([-1, -8, -9, 7, 8, 32767, -32767, -32768, I32MAX, I32MIN, 0, 3], np.int64)
        for k in range(4):
            yield ("vectors%d-%s" % (k, tag), _planes(rng, W, H, bpp, sh, sv), _planes(rng, W, H, bpp, sh, sv),
                   _acc(GW, GH, V[cells % 12], V[(cells // 2 + 3 * k) % 12], 9, hops=65535, end=NOFIELD), 9, W, H, bpp, sh, sv)
    # which cells apply: hops 0 with the root, another root, root 0 with each end code, and cells that do
    a = _acc(GW, GH, 9, -5, 7, hops=2)
    a["hops"][0, :] = 0                                          # intra cells of a frame whose serial is b's
    a["root"][1, :3] = 8                                         # chains that ended in another frame
    a["root"][1, 3:], a["end"][1, 3:] = 0, NOFIELD
    a["root"][2, :3], a["end"][2, :3] = 0, SCALED
    a["root"][2, 3:], a["end"][2, 3:] = 0, INTRA
    for sb in (7, 8, 6):
        yield ("applies-b%d" % sb, _planes(rng, W, H, 8, 1, 1), _planes(rng, W, H, 8, 1, 1), a.copy(), sb, W, H, 8, 1, 1)
    # 1 sample wide, odd and not a multiple of the cell, pitched with poison beyond the width
    for w, h, sh, sv, bpp in ((1, 1, 1, 1, 8), (1, 7, 0, 0, 8), (5, 3, 1, 1, 8), (5, 3, 1, 0, 10), (66, 66, 1, 1, 8),
                              (66, 34, 0, 1, 10)):
        gw, gh = 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)
        dx, dy = rng.integers(-8 * w - 9, 8 * w + 9, (gh, gw)), rng.integers(-8 * h - 9, 8 * h + 9, (gh, gw))
        root = np.where(rng.random((gh, gw)) < 0.8, 4, 3)
        yield ("size%dx%d-%d%d-%dbit" % (w, h, sh, sv, bpp), _planes(rng, w, h, bpp, sh, sv, pad=3, poison=0x5a),
               _planes(rng, w, h, bpp, sh, sv, pad=5, poison=0xa5), _acc(gw, gh, dx, dy, root), 4, w, h, bpp, sh, sv)
    # the int16 clamp of the residual: stored 16-bit codes beyond the depth
    full, none = [np.full(s, 65535, np.uint16) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))], None
    none = [np.zeros_like(x) for x in full]
    yield ("clamp-high", full, none, _acc(GW, GH, 0, 0, 2), 2, W, H, 10, 1, 1)
    yield ("clamp-low", none, full, _acc(GW, GH, 3, -3, 2), 2, W, H, 10, 1, 1)


MODES = [(i, o) for i in ("nearest", "bilinear") for o in ("residual", "picture")]


@pytest.fixture(scope="module")
def cases():
    return list(hand_cases())


def test_host_equals_the_restatement(v9, cases):
    for name, A, B, acc, sb, w, h, bpp, sh, sv in cases:
        for interp, output in MODES:
            want, wmask = warp_ref(A, B, acc, sb, w, h, sh, sv, interp, output)
            got = v9.acc_warp_host(A, B, acc, sb, w, h, bpp, sh, sv, output=output, interp=interp, mask=True)
            for p in range(3):
                assert got[p].dtype == np.int16 and got[p].shape == want[p].shape
                assert np.array_equal(got[p], want[p]), "%s %s %s plane %d: %d samples differ" % (
                    name, interp, output, p, int((got[p] != want[p]).sum()))
            assert got[3].dtype == np.uint8 and np.array_equal(got[3], wmask), name
            assert len(v9.acc_warp_host(A, B, acc, sb, w, h, bpp, sh, sv, output=output, interp=interp)) == 3


def test_the_cases_cover_what_they_claim(cases):
    """From the restatement alone: the phases, the four edges, the vectors and the apply rule."""
    by = {}
    for name, A, B, acc, sb, w, h, bpp, sh, sv in cases:
        by.setdefault(re.match("[a-z]+", name).group(), []).append(warp_stats(acc, sb, w, h, sh, sv) | dict(sh=sh, acc=acc))
    even = {(x, y) for x in range(0, 16, 2) for y in range(0, 16, 2)}
    every = {(x, y) for x in range(16) for y in range(16)}
    luma = set().union(*[s["luma_phases"] for s in by["phases"]])
    c420 = set().union(*[s["chroma_phases"] for s in by["phases"] if s["sh"]])
    c444 = set().union(*[s["chroma_phases"] for s in by["phases"] if not s["sh"]])
    assert luma == even and c444 == even and c420 == every
    for kind in ("phases", "vectors", "size"):
        assert np.logical_or.reduce([s["sides"] for s in by[kind]]).all(), kind
    seen = set(np.concatenate([s["acc"]["dx"].ravel() for s in by["vectors"]]).tolist())
    assert {-1, -8, -9, 7, 8, 32767, -32767, -32768, I32MAX, I32MIN} <= seen
    assert all(s["applying"] == 1.0 for s in by["vectors"])
    assert [round(s["applying"] * 24) for s in by["applies"]] == [6, 3, 0]


def test_nearest_rounds_half_up_and_negative_vectors_floor(v9):
    """-1, -8, -9, 7, 8 in 1/8 luma sample on a ramp: the sample each lands on, by hand."""
    ramp = np.arange(W, dtype=np.uint8)[None, :].repeat(H, 0) * 4
    cr = np.arange(W // 2, dtype=np.uint8)[None, :].repeat(H // 2, 0) * 8
    A = [np.zeros_like(ramp), np.zeros_like(cr), np.zeros_like(cr)]
    for vx, luma_step, chroma_step in ((-1, 0, 0), (-8, -1, 0), (-9, -1, -1), (7, 1, 0), (8, 1, 1), (4, 1, 0), (-4, 0, 0),
                                       (-12, -1, -1)):
        # luma (2 vx + 8) >> 4, 4:2:0 chroma (vx + 8) >> 4
        assert (2 * vx + 8) >> 4 == luma_step and (vx + 8) >> 4 == chroma_step
        y, u, v = v9.acc_warp_host(A, [ramp, cr, cr], _acc(GW, GH, vx, 0, 1), 1, W, H, 8, output="picture")
        assert y[0, 8] == 4 * (8 + luma_step) and u[0, 4] == 8 * (4 + chroma_step) and v[3, 4] == u[0, 4]
        y, u, v = v9.acc_warp_host(A, [ramp, cr, cr], _acc(GW, GH, vx, 0, 1), 1, W, H, 8, output="picture", interp="bilinear")
        # on a ramp the bilinear value is the ramp at the displaced position, rounded: 4 (8 + vx / 8) + 0.5
        assert y[0, 8] == (4 * 16 * 8 + 4 * 2 * vx + 8) >> 4


def test_bad_arguments(v9):
    rng = np.random.default_rng(5)
    A, B, acc = _planes(rng, W, H, 8, 1, 1), _planes(rng, W, H, 8, 1, 1), _acc(GW, GH, 0, 0, 1)
    for kw in (dict(output="sum"), dict(interp="cubic")):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.acc_warp_host(A, B, acc, 1, W, H, 8, **kw)
        assert e.value.code == v9.EINVAL
    with pytest.raises(v9.Vp9HipError) as e:
        v9.acc_warp_host(_planes(rng, W, H, 10, 1, 1), _planes(rng, W, H, 10, 1, 1), acc, 1, W, H, 9)
    assert e.value.code == v9.EINVAL
    for size in ((0, 8), (8, 0), (16385, 8)):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.warp_layout(*size)
        assert e.value.code == v9.EINVAL
    with pytest.raises(v9.Vp9HipError):
        v9.warp_layout(8, 8, 2, 0)
    assert v9.warp_layout(66, 34, 1, 1) == (2 * (66 * 34 + 2 * 33 * 17), (0, 2 * 66 * 34, 2 * (66 * 34 + 33 * 17)))
    assert v9.warp_layout(5, 3, 1, 0) == (2 * (15 + 2 * 9), (0, 30, 48))
    assert v9.warp_layout(5, 3, 0, 0)[0] == 90
