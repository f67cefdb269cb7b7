"""Accumulated motion: a numpy restatement of the definition in include/vp9hip.h ("accumulated
motion"), sharing no code with the library, against vp9hip_motion_acc_host (CPU suite).

acc_frame / acc_chain below are what tests/test_gpu_motion_acc.py compares the kernel with.
Hand-made fields on a 6 x 4 grid pin the rounding, the clamps, the end codes, the wrap and the
saturation; synthetic key + 6 inter chains pin the recurrence over real block layouts.
"""
import numpy as np
import pytest

from test_motion_definition import motion_field

INTRA, NOFIELD, SCALED = 0, 1, 2
CELL = np.dtype([("dx", "<i4"), ("dy", "<i4"), ("root", "<u4"), ("hops", "<u2"), ("end", "u1"), ("pad", "u1")])


def acc_frame(mv, info, serial, parents, parent_end=(NOFIELD,) * 3):
    """One frame of the recurrence: mv (GH, GW, 2, 2), info (GH, GW, 4), parents[k] a CELL array
    of the same grid or None, when parent_end[k] says why. Returns (CELL array, cells whose
    parent cell was clamped)."""
    gh, gw = info.shape[:2]
    out = np.zeros((gh, gw), CELL)
    clamped = np.zeros((gh, gw), bool)
    for r in range(gh):
        for c in range(gw):
            i0 = int(info[r, c, 0])
            if i0 == 255:
                out[r, c] = (0, 0, serial, 0, INTRA, 0)
                continue
            mx, my = int(mv[r, c, 0, 0]), int(mv[r, c, 0, 1])
            if i0 > 2 or parents[i0] is None:
                out[r, c] = (mx, my, 0, 1, NOFIELD if i0 > 2 else parent_end[i0], 0)
                continue
            fc, fr = (32 * c + 16 + mx) // 32, (32 * r + 16 + my) // 32      # Python's // floors
            pc, pr = min(max(fc, 0), gw - 1), min(max(fr, 0), gh - 1)
            clamped[r, c] = (pc, pr) != (fc, fr)
            q = parents[i0][pr, pc]
            wrap = lambda v: (v + 2 ** 31) % 2 ** 32 - 2 ** 31               # noqa: E731
            out[r, c] = (wrap(mx + int(q["dx"])), wrap(my + int(q["dy"])), q["root"], min(int(q["hops"]) + 1, 65535),
                         q["end"], 0)
    return out, clamped


def acc_chain(fields, parent_of, serial0=1):
    """The recurrence over a list of (mv, info) in decode order; parent_of(t) -> per name the
    index of the parent frame, or None / (None, end). Returns the CELL arrays and clamp masks."""
    out, cl = [], []
    for t, (mv, info) in enumerate(fields):
        par, end = [None] * 3, [NOFIELD] * 3
        for k, p in enumerate(parent_of(t)):
            if isinstance(p, tuple):
                end[k] = p[1]
            elif p is not None:
                par[k] = out[p]
        a, c = acc_frame(mv, info, serial0 + t, par, end)
        out.append(a)
        cl.append(c)
    return out, cl


def gop_parents(t):
    """LAST = t - 1, GOLDEN = 0, ALTREF = max(t - 2, 0); the key frame has none."""
    return (None,) * 3 if t == 0 else (t - 1, 0, max(t - 2, 0))


def gop_frames(v9, w, h, n=7, seed=7100, **kw):
    kw = dict(dict(mv_range=64, ref_mix=0), **kw)
    return [v9.SynthFrame(v9.synth_params(w, h, 8, seed=seed + t, inter=int(t > 0), compound=int(t > 1), **kw))
            for t in range(n)]


def gop_fields(frames):
    out = []
    for f in frames:
        mv, info, hits = motion_field(f.blocks(), f.pkt.width, f.pkt.height)
        assert hits.min() == 1 and hits.max() == 1
        out.append((mv, info))
    return out


def _host(v9, mv, info, serial, parents, ends=(NOFIELD,) * 3):
    got = v9.motion_acc_host(mv, info, serial, parents, ends)
    assert got.dtype == v9.ACC_CELL and v9.ACC_CELL == CELL
    return got


GW, GH = 6, 4


def _field(i0=0, mx=0, my=0, i1=255):
    mv, info = np.zeros((GH, GW, 2, 2), np.int16), np.zeros((GH, GW, 4), np.uint8)
    info[..., 0], info[..., 1] = i0, i1
    mv[..., 0, 0], mv[..., 0, 1] = mx, my
    return mv, info


def _both(v9, mv, info, serial, parents, ends=(NOFIELD,) * 3):
    want, _ = acc_frame(mv, info, serial, parents, ends)
    got = _host(v9, mv, info, serial, parents, ends)
    assert got.tobytes() == want.tobytes()
    return got


def test_uniform_motion_sums_and_clamps_at_the_right_edge(v9):
    key = _both(v9, *_field(255), 1, [None] * 3)
    assert (key["root"] == 1).all() and (key["hops"] == 0).all() and (key["end"] == INTRA).all()
    a = key
    for t in (2, 3, 4):
        a = _both(v9, *_field(0, mx=32), t, [a, None, None])
    # three frames each one cell to the right: 96 everywhere, the chain pinned to the last column
    assert (a["dx"] == 96).all() and (a["dy"] == 0).all() and (a["hops"] == 3).all() and (a["root"] == 1).all()
    mark = np.zeros((GH, GW), CELL)
    mark["dx"] = np.arange(GW)[None, :] * 1000
    b = _both(v9, *_field(0, mx=32), 5, [mark, None, None])
    assert (b["dx"][:, :-1] == 32 + 1000 * np.arange(1, GW)).all()
    assert (b["dx"][:, -1] == 32 + 1000 * (GW - 1)).all()                 # clamped: its own column


def test_rounding_floors(v9):
    mark = np.zeros((GH, GW), CELL)
    mark["root"] = 100 + np.arange(GW)[None, :] + 10 * np.arange(GH)[:, None]
    for m, step in ((-1, 0), (-16, 0), (-17, -1), (15, 0), (16, 1), (-48, -1), (-49, -2)):
        a = _both(v9, *_field(0, mx=m), 9, [mark, None, None])
        assert a["root"][1, 3] == mark["root"][1, 3 + step], (m, step)
        b = _both(v9, *_field(0, my=m), 9, [mark, None, None])
        assert b["root"][2, 3] == mark["root"][2 + step, 3], (m, step)


def test_compound_second_vector_is_ignored_and_unknown_names_end(v9):
    mv, info = _field(1, mx=40, my=-40, i1=2)
    mv[..., 1, :] = 0x7fff                                                # poisoned
    mark = np.zeros((GH, GW), CELL)
    mark["dx"], mark["hops"], mark["root"] = 7, 2, 55
    poison = np.zeros((GH, GW), CELL)
    poison["dx"] = 123456
    a = _both(v9, mv, info, 9, [poison, mark, poison])
    assert (a["dx"] == 47).all() and (a["dy"] == -40).all() and (a["hops"] == 3).all() and (a["root"] == 55).all()
    info[..., 0] = 7
    a = _both(v9, mv, info, 9, [mark, mark, mark])
    assert (a["end"] == NOFIELD).all() and (a["hops"] == 1).all() and (a["root"] == 0).all() and (a["dx"] == 40).all()
    a = _both(v9, *_field(2, mx=3), 9, [mark, mark, None], (NOFIELD, NOFIELD, SCALED))
    assert (a["end"] == SCALED).all() and (a["hops"] == 1).all() and (a["dx"] == 3).all()


def test_saturation_and_wrap(v9):
    q = np.zeros((GH, GW), CELL)
    q["hops"], q["dx"], q["dy"], q["end"], q["root"] = 65535, 2 ** 31 - 1, -2 ** 31, SCALED, 2 ** 32 - 1
    a = _both(v9, *_field(0, mx=1, my=-1), 9, [q, None, None])
    assert (a["hops"] == 65535).all() and (a["dx"] == -2 ** 31).all() and (a["dy"] == 2 ** 31 - 1).all()
    assert (a["end"] == SCALED).all() and (a["root"] == 2 ** 32 - 1).all()
    q["hops"] = 65534
    assert (_both(v9, *_field(0), 9, [q, None, None])["hops"] == 65535).all()


def test_bad_arguments(v9):
    mv, info = _field(0)
    with pytest.raises(v9.Vp9HipError) as e:
        v9.motion_acc_host(mv, info, 1, [None] * 3, (INTRA, NOFIELD, NOFIELD))
    assert e.value.code == v9.EINVAL
    with pytest.raises(v9.Vp9HipError) as e:
        v9.motion_acc_host(mv[:, :3], info, 1)
    assert e.value.code == v9.EINVAL
    with pytest.raises(v9.Vp9HipError) as e:
        v9.motion_acc_host(mv, info, 1, [np.zeros((GH, GW + 1), CELL), None, None])
    assert e.value.code == v9.EINVAL


@pytest.mark.parametrize("w,h", [(66, 66), (200, 130)])
def test_synthetic_chain(v9, w, h):
    fields = gop_fields(gop_frames(v9, w, h))
    want, clamped = acc_chain(fields, gop_parents)
    # the reference alone: the chains are long, and some cell clamps
    deep = float((want[-1]["hops"] == 6).mean())
    print("%dx%d: %.2f of the last frame's cells have hops == 6, %d clamped cells" % (w, h, deep, sum(int(c.sum()) for c in clamped)))
    assert deep >= 0.25
    assert any(c.any() for c in clamped)
    got = []
    for t, (mv, info) in enumerate(fields):
        par = [None if p is None else got[p] for p in gop_parents(t)]
        got.append(_host(v9, mv, info, 1 + t, par))
        assert got[t].tobytes() == want[t].tobytes(), "frame %d differs in %d cells" % (t, int((got[t] != want[t]).sum()))
