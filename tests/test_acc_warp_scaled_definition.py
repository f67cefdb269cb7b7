"""Accumulated residual at model size: the host statement (vp9hip_acc_warp_scaled_host,
csrc/host/vp9h_warp_scaled.c) against the composition of the two numpy restatements the
definition in include/vp9hip.h ("accumulated residual at model size") composes: warp_ref of
tests/test_acc_warp_definition.py, then ref_tensor of tests/test_residual_scaled_definition.py; the
coverage is sbox of the mask widened to luma samples times 256. The reference shares no code with
the library. CPU only; every comparison is exact, halves by bit pattern.

ref_scaled / coverage_ref below are what tests/test_gpu_acc_warp_scaled.py compares the kernel
with. What the inputs exercise is asserted first, from the reference alone.
"""
import ctypes

import numpy as np
import pytest

from test_acc_warp_definition import hand_cases, warp_ref
from test_gpu_convert_scale import _weights
from test_motion_acc_definition import CELL
from test_residual_scaled_definition import MATRICES, bits, ref_tensor, resampled, same, sbox

FORMATS = ["yuv_i16", "yuv_f16", "rgb_i16", "rgb_f16"]
INTERPS = ["nearest", "bilinear"]
SIZES = [None, (1, 1), (5, 3), (7, 16), (24, 16), (49, 20)]


# ------------------------------------------------------------------ the reference
def coverage_ref(mask, w, h, ow, oh, fmt):
    """The fourth plane: sbox(256 applies(cell of the luma sample)) as the format stores it."""
    dense = np.repeat(np.repeat(mask.astype(np.int64) * 256, 4, 0), 4, 1)[:h, :w]
    c = sbox(dense, ow, oh)
    assert c.min() >= 0 and c.max() <= 256
    if fmt.endswith("f16"):
        return (c.astype(np.float32) * np.float32(1.0 / 256)).astype(np.float16)
    return c.astype(np.int16)


def ref_scaled(R, mask, w, h, sh, sv, bpp, fmt, ow, oh, cs=2, full=0, coverage=False, pre=None):
    """The (3 or 4, OH, OW) tensor of one pair from warp_ref's residual planes R and mask."""
    t = ref_tensor(R, w, h, sh, sv, bpp, fmt, ow, oh, cs, full, pre)
    if coverage:
        t = np.concatenate([t, coverage_ref(mask, w, h, ow, oh, fmt)[None]])
    return t


def half_case():
    """2 x 2 at 4:4:4 whose four residuals are (-3, -2, -3, -2): at (1, 1) the mean is -2.5 -> -2,
    the floor that separates sbox from rounding half away from zero."""
    A = [np.zeros((2, 2), np.uint8) for _ in range(3)]
    B = [np.array([[3, 2], [3, 2]], np.uint8) for _ in range(3)]
    acc = np.zeros((2, 2), CELL)
    acc["root"], acc["hops"] = 1, 1
    return ("half-444-8bit", A, B, acc, 1, 2, 2, 8, 0, 0)


def all_cases():
    return list(hand_cases()) + [half_case()]


@pytest.fixture(scope="module")
def cases():
    """Every case with warp_ref's result for both modes, computed once."""
    out = []
    for case in all_cases():
        name, A, B, acc, sb, w, h, bpp, sh, sv = case
        out.append((case, {i: warp_ref(A, B, acc, sb, w, h, sh, sv, i, "residual") for i in INTERPS}))
    return out


# ------------------------------------------------------------------ what the inputs exercise, from the reference alone
def test_the_cases_exercise_what_they_claim(cases):
    by = {c[0]: (c, refs) for c, refs in cases}
    # coverage: 96, 48 and 0 applying luma samples of 384 -> floor((256 n + 192) / 384)
    for name, n, want in (("applies-b7", 96, 64), ("applies-b8", 48, 32), ("applies-b6", 0, 0)):
        (_, A, B, acc, sb, w, h, bpp, sh, sv), refs = by[name]
        mask = refs["nearest"][1]
        assert int(mask.sum()) * 16 == n and (256 * n + 192) // 384 == want
        assert coverage_ref(mask, w, h, 1, 1, "yuv_i16").tolist() == [[want]]
        assert coverage_ref(mask, w, h, 1, 1, "yuv_f16").tolist() == [[want / 256]]
        c = coverage_ref(mask, w, h, 5, 3, "yuv_i16")
        if n:
            assert ((c > 0) & (c < 256)).any() and (c == 0).any(), name
        else:
            assert (c == 0).all()
    # the int16 extremes of the residual survive the mean, and the RGB formats clip them to +-m
    for name, v in (("clamp-high", 32767), ("clamp-low", -32768)):
        (_, A, B, acc, sb, w, h, bpp, sh, sv), refs = by[name]
        R, mask = refs["bilinear"]
        m = (1 << bpp) - 1
        assert (ref_scaled(R, mask, w, h, sh, sv, bpp, "yuv_i16", 5, 3) == v).all()
        rgb = ref_scaled(R, mask, w, h, sh, sv, bpp, "rgb_i16", 5, 3)
        assert (rgb == (m if v > 0 else -m)).all(), name
    # a negative mean with a fractional part of exactly one half: -10 / 4 -> -2
    (_, A, B, acc, sb, w, h, bpp, sh, sv), refs = by["half-444-8bit"]
    R, mask = refs["nearest"]
    assert R[0].tolist() == [[-3, -2], [-3, -2]] and int(R[0].sum()) == -10
    assert ref_scaled(R, mask, w, h, sh, sv, bpp, "yuv_i16", 1, 1).ravel().tolist() == [-2, -2, -2]
    # and whether the hand-made cases of the older test give such a mean too (printed, not needed)
    found = 0
    for (name, A, B, acc, sb, w, h, bpp, sh, sv), refs in cases[:-1]:
        for ow, oh in ((1, 1), (5, 3), (7, 16)):
            Aw = _weights(h, oh) @ refs["nearest"][0][0].astype(np.int64) @ _weights(w, ow).T
            found += int(((Aw < 0) & ((2 * Aw) % (2 * w * h) == w * h)).sum())
    print("negative half-way luma means among the older hand cases: %d" % found)


def test_444_identity(v9, cases):
    """resize=None at 4:4:4, "yuv_i16": warp_ref's three planes unchanged."""
    seen = 0
    for (name, A, B, acc, sb, w, h, bpp, sh, sv), refs in cases:
        if sh or sv:
            continue
        for interp in INTERPS:
            got = v9.acc_warp_scaled_host(A, B, acc, sb, w, h, bpp, sh, sv, "yuv_i16", None, interp=interp)
            same(got, np.stack(refs[interp][0]), "%s %s identity" % (name, interp))
            seen += 1
    assert seen >= 60


# ------------------------------------------------------------------ the host statement against the reference
def test_host_statement_equals_the_composition(v9, cases):
    for k, ((name, A, B, acc, sb, w, h, bpp, sh, sv), refs) in enumerate(cases):
        all_matrices = sh == 1 and sv == 1 and name.startswith(("phases0-", "vectors0-"))
        assert not all_matrices or bpp in (8, 10)
        for interp in INTERPS:
            R, mask = refs[interp]
            for j, size in enumerate(SIZES):
                ow, oh = size or (w, h)
                pre = resampled(R, w, h, sh, sv, ow, oh)
                for f, fmt in enumerate(FORMATS):
                    mats = MATRICES if all_matrices and fmt.startswith("rgb") and size == (5, 3) else [(2, 0)]
                    for cs, full in mats:
                        cov = bool((k + j + f) & 1)
                        got = v9.acc_warp_scaled_host(A, B, acc, sb, w, h, bpp, sh, sv, fmt, size, interp=interp, coverage=cov,
                                                      colorspace=cs, full_range=full)
                        want = ref_scaled(R, mask, w, h, sh, sv, bpp, fmt, ow, oh, cs, full, cov, pre)
                        same(got, want, "%s %s %s -> %s cs %d full %d coverage %d" % (name, interp, fmt, size, cs, full, cov))


def test_host_statement_equals_the_two_older_host_statements(v9, cases):
    """residual_scaled_host(acc_warp_host(...)): the composition in the library's own C."""
    for (name, A, B, acc, sb, w, h, bpp, sh, sv), _ in cases:
        for interp in INTERPS:
            planes = v9.acc_warp_host(A, B, acc, sb, w, h, bpp, sh, sv, output="residual", interp=interp)
            for fmt, size in (("yuv_i16", (5, 3)), ("rgb_f16", (7, 16)), ("rgb_i16", None), ("yuv_f16", (49, 20))):
                got = v9.acc_warp_scaled_host(A, B, acc, sb, w, h, bpp, sh, sv, fmt, size, interp=interp)
                same(got, v9.residual_scaled_host(planes, w, h, sh, sv, bpp, fmt, size), "%s %s %s -> %s" % (name, interp, fmt, size))


# ------------------------------------------------------------------ layout, pitched outputs, refusals
def _raw_call(v9, case, desc, dst, a=True, b=True, la=True, lb=True, field=True, bpp=None, sh=None, sv=None, hole=False):
    name, A, B, acc, sb, w, h, d, ssh, ssv = case
    keep = [np.ascontiguousarray(p) for p in A] + [np.ascontiguousarray(p) for p in B]
    ap = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in keep[:3]])
    bp = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in keep[3:]])
    if hole:
        ap[1] = None
    ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in keep[:3]])
    cells = np.ascontiguousarray(acc, v9.ACC_CELL)
    return v9.lib().vp9hip_acc_warp_scaled_host(
        ctypes.byref(ap) if a else None, ctypes.byref(ls) if la else None, ctypes.byref(bp) if b else None,
        ctypes.byref(ls) if lb else None, cells.ctypes.data if field else None, sb, d if bpp is None else bpp,
        ssh if sh is None else sh, ssv if sv is None else sv, ctypes.byref(desc) if desc is not None else None, dst)


def test_layout_and_pitched_outputs(v9, cases):
    assert v9.warpt_layout("rgb_f16", (33, 17)) == (3 * 66 * 17, 66)
    assert v9.warpt_layout("rgb_f16", (33, 17), coverage=True) == (4 * 66 * 17, 66)
    assert v9.warpt_layout("yuv_i16", (33, 17), coverage=True, pitch=80) == (4 * 80 * 17, 80)
    assert v9.warpt_layout("yuv_i16", (33, 17), pitch=66, frame_stride=3 * 66 * 17 + 2)[0] == 3 * 66 * 17
    for kw in (dict(resize=(0, 17)), dict(resize=(16385, 17)), dict(resize=(33, 0)), dict(resize=(33, 16385)), dict(pitch=64),
               dict(pitch=72), dict(pitch=-16), dict(frame_stride=3 * 66 * 17 - 2), dict(frame_stride=3 * 66 * 17 + 1),
               dict(frame_stride=-2), dict(coverage=True, frame_stride=3 * 66 * 17)):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.warpt_layout("yuv_i16", **dict(dict(resize=(33, 17)), **kw))
        assert e.value.code == v9.EINVAL, kw
    pitch = ctypes.c_int64()
    for planes in (2, 5, 0, -3):
        d = v9.WarptDesc(0, 2, 0, 0, planes, 8, 8, 4, 4, 0, 0)
        assert v9.lib().vp9hip_warpt_layout(ctypes.byref(d), ctypes.byref(pitch)) == v9.EINVAL
    for fmt in (-1, 4):
        d = v9.WarptDesc(fmt, 2, 0, 0, 3, 8, 8, 4, 4, 0, 0)
        assert v9.lib().vp9hip_warpt_layout(ctypes.byref(d), ctypes.byref(pitch)) == v9.EINVAL
    assert v9.lib().vp9hip_warpt_layout(None, None) == v9.EINVAL
    # a pitched, strided output: the rows are the tight call's, the bytes between them untouched
    case = next(c for c, _ in cases if c[0] == "size66x34-01-10bit")
    name, A, B, acc, sb, w, h, bpp, sh, sv = case
    for fmt, cov in (("rgb_i16", True), ("yuv_f16", False)):
        tight = v9.acc_warp_scaled_host(A, B, acc, sb, w, h, bpp, sh, sv, fmt, (5, 3), interp="bilinear", coverage=cov)
        P = 4 if cov else 3
        d = v9.WarptDesc(v9.RESID_FORMATS[fmt], 2, 0, 1, P, w, h, 5, 3, 32, P * 32 * 3 + 6)
        buf = np.full(P * 16 * 3 + 8, 0x5a5a, np.int16)
        assert _raw_call(v9, case, d, buf.ctypes.data) == 0
        rows = buf[:P * 16 * 3].reshape(P, 3, 16)
        assert np.array_equal(rows[:, :, :5], bits(tight)) and (rows[:, :, 5:] == 0x5a5a).all() and (buf[P * 48:] == 0x5a5a).all()


def test_host_statement_refuses(v9, cases):
    case = next(c for c, _ in cases if c[0] == "phases0-420-8bit")
    out = np.full(4 * 4 * 4 + 8, 0x5a5a, np.int16)

    def call(fmt=2, cs=2, mode=0, planes=4, w=24, h=16, ow=4, oh=4, p=0, fs=0, dst=None, desc=True, **kw):
        d = v9.WarptDesc(fmt, cs, 0, mode, planes, w, h, ow, oh, p, fs) if desc else None
        return _raw_call(v9, case, d, out.ctypes.data if dst is None else dst, **kw)
    assert call() == 0 and (out[:64] != 0x5a5a).any() and (out[64:] == 0x5a5a).all()
    out[:] = 0x5a5a
    for kw in (dict(w=0), dict(w=16385), dict(h=0), dict(h=16385), dict(sh=2), dict(sv=-1), dict(bpp=9), dict(bpp=16),
               dict(fmt=-1), dict(fmt=4), dict(cs=0), dict(cs=6), dict(cs=8), dict(cs=-1), dict(fmt=3, cs=0),
               dict(mode=-1), dict(mode=2), dict(planes=2), dict(planes=5), dict(planes=0),
               dict(ow=0), dict(ow=16385), dict(oh=0), dict(oh=16385), dict(p=6), dict(p=24), dict(p=-16), dict(fs=126),
               dict(fs=129), dict(fs=-2), dict(dst=out.ctypes.data + 1), dict(dst=None, desc=False), dict(a=False), dict(b=False),
               dict(la=False), dict(lb=False), dict(field=False), dict(hole=True)):
        assert call(**kw) == v9.EINVAL, kw
    assert _raw_call(v9, case, v9.WarptDesc(2, 2, 0, 0, 4, 24, 16, 4, 4, 0, 0), None) == v9.EINVAL
    assert (out == 0x5a5a).all()
    assert call(fmt=0, cs=0) == 0                  # the YUV formats do not look at the colour space
    name, A, B, acc, sb, w, h, bpp, sh, sv = case
    for kw in (dict(fmt="rgb_u8"), dict(interp="cubic")):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.acc_warp_scaled_host(A, B, acc, sb, w, h, bpp, sh, sv, **dict(dict(fmt="rgb_i16", resize=(4, 4)), **kw))
        assert e.value.code == v9.EINVAL
    with pytest.raises(v9.Vp9HipError) as e:
        v9.acc_warp_scaled_host(A, B, acc, sb, w, h, bpp, sh, sv, "rgb_i16", (4, 4), colorspace=6)
    assert e.value.code == v9.EINVAL
    with pytest.raises(v9.Vp9HipError):
        v9.acc_warp_scaled_host(A, B, acc, sb, w, h, bpp, sh, sv, "rgb_i16", (0, 4))
    with pytest.raises(ValueError):
        v9.acc_warp_scaled_host(A, B, acc, sb, 2 * w, h, bpp, sh, sv, "rgb_i16", (4, 4))      # planes smaller than the size
