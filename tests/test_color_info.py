"""The stream's colour description through the host parse, and the host-only helpers of the
output conversion (include/vp9hip.h: vp9h_stream_set_color, vp9h_frame_info.colorspace /
full_range, vp9hip_out_coefs, vp9hip_out_layout). CPU only.

read_colorspace_details (vp9.c:457-517) stores the 3-bit colour space and the range bit in
avctx->colorspace / color_range, where they persist over inter frames and
show_existing_frame; RGB (code 7) has no range bit and is full range; an intra-only frame
in profile 0 codes no colour config and is BT.601 limited, 8-bit 4:2:0.
"""
import math

import pytest

from test_stream import _frames

KR_KB = {1: (.299, .114), 2: (.2126, .0722), 3: (.299, .114), 4: (.212, .087), 5: (.2627, .0593)}


def _encode(v9, enc, frames, show_existing=True):
    """Keyframe + inter frames on LAST = the previous frame, then a show_existing_frame."""
    datas = [enc.encode(frames[0])[0]]
    for i in range(1, len(frames)):
        datas.append(enc.encode(frames[i], ref_slot=(i - 1, 0, i - 1), refresh_mask=1 << i)[0])
    if show_existing:
        datas.append(enc.encode(None, show_existing_frame=1, show_slot=1)[0])
    return datas


@pytest.fixture(scope="module")
def gop(v9):
    return _frames(v9, 64, 64, 3)


@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("cs", [0, 1, 2, 3, 4, 5])
def test_color_round_trips_on_every_frame(v9, gop, cs, full):
    enc = v9.Stream()
    enc.set_color(cs, full)
    datas = _encode(v9, enc, gop)
    dec = v9.Stream()
    infos = [dec.decode(d)[1] for d in datas]
    assert [i.show_existing_frame for i in infos] == [0, 0, 0, 1]
    assert [(i.colorspace, i.full_range) for i in infos] == [(cs, full)] * 4
    t, peek = v9.frame_peek(datas[0])
    assert t == 0 and (peek.colorspace, peek.full_range) == (cs, full)
    t, peek = v9.frame_peek(datas[1])              # an inter header codes no colour: stateless peek leaves 0
    assert t == 1 and (peek.colorspace, peek.full_range) == (0, 0)


def test_rgb_is_444_and_full_range(v9):
    f444 = _frames(v9, 64, 64, 2, ss_h=0, ss_v=0)
    enc = v9.Stream()
    enc.set_color(7, 0)
    datas = _encode(v9, enc, f444, show_existing=False)
    dec = v9.Stream()
    for d in datas:
        p, info = dec.decode(d)
        assert (info.colorspace, info.full_range) == (7, 1)
        assert (p.pkt.ss_h, p.pkt.ss_v, p.pkt.bpp) == (0, 0, 8)
    assert tuple(getattr(v9.frame_peek(datas[0])[1], k) for k in ("colorspace", "full_range")) == (7, 1)
    # 10-bit 4:4:4 is profile 3
    f3 = _frames(v9, 64, 64, 1, bpp=10, ss_h=0, ss_v=0)
    enc = v9.Stream()
    enc.set_color(7, 1)
    p, info = v9.Stream().decode(enc.encode(f3[0])[0])
    assert (info.colorspace, info.full_range, p.pkt.bpp) == (7, 1, 10)


def test_rgb_needs_444_and_code_6_is_reserved(v9, gop):
    enc = v9.Stream()
    enc.set_color(7, 1)
    with pytest.raises(v9.Vp9HipError) as e:
        enc.encode(gop[0])                          # 4:2:0
    assert e.value.code == v9.EINVAL
    f422 = _frames(v9, 64, 64, 1, ss_h=1, ss_v=0)
    with pytest.raises(v9.Vp9HipError) as e:
        enc.encode(f422[0])
    assert e.value.code == v9.EINVAL
    for bad in (6, 8, -1):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.Stream().set_color(bad, 0)
        assert e.value.code == v9.EINVAL


def test_default_bitstream_is_bt709_limited(v9, gop):
    """Without set_color the encoder writes what it always wrote: colour space 2, range 0
    (byte 4 of a profile-0 keyframe: 8 header bits, the 24-bit sync code, then the 3-bit colour
    space and the range bit), and set_color(2, 0) is the same stream byte for byte."""
    plain = _encode(v9, v9.Stream(), gop)
    assert plain[0][1:4] == b"\x49\x83\x42" and plain[0][4] >> 4 == 0b0100
    enc = v9.Stream()
    enc.set_color(2, 0)
    assert _encode(v9, enc, gop) == plain
    enc = v9.Stream()
    enc.set_color(5, 1)
    other = _encode(v9, enc, gop)
    assert other[0][4] >> 4 == 0b1011 and other[0][:4] == plain[0][:4]
    assert bytes([other[0][4] & 15]) + other[0][5:] == bytes([plain[0][4] & 15]) + plain[0][5:]
    assert other[1:] == plain[1:]                   # inter frames and show_existing code no colour
    dec = v9.Stream()
    for d in plain:
        info = dec.decode(d)[1]
        assert (info.colorspace, info.full_range) == (2, 0)
    peek = v9.frame_peek(plain[0])[1]
    assert (peek.colorspace, peek.full_range) == (2, 0)


def test_intra_only_profile_0_is_bt601_limited(v9, gop):
    enc = v9.Stream()
    enc.set_color(5, 1)
    key = enc.encode(gop[0])[0]
    intra = v9.SynthFrame(v9.synth_params(64, 64, 8, seed=77))
    intra.pkt.keyframe, intra.pkt.intraonly = 0, 1
    io = enc.encode(intra, show_frame=0, refresh_mask=0x24)[0]
    dec = v9.Stream()
    info = dec.decode(key)[1]
    assert (info.colorspace, info.full_range) == (5, 1)
    p, info = dec.decode(io)
    assert p.pkt.intraonly and (p.pkt.bpp, p.pkt.ss_h, p.pkt.ss_v) == (8, 1, 1)
    assert (info.colorspace, info.full_range) == (1, 0)
    t, peek = v9.frame_peek(io)                    # the header codes no colour: the stateless peek leaves 0
    assert t == 3 and (peek.colorspace, peek.full_range) == (0, 0)


def _coefs(cs, full, d, o):
    """vp9hip_out_coefs restated: floor(x * 2^S + 0.5) in double."""
    kr, kb = KR_KB[cs]
    s = 14 + d - o
    m = float((1 << o) - 1)
    up = float(1 << (d - 8))
    sy = m / float((1 << d) - 1) if full else m / (219. * up)
    sc = m / float((1 << d) - 1) if full else m / (224. * up)
    kg = 1. - kr - kb
    x = (sy, 2. * (1. - kr) * sc, 2. * kb * (1. - kb) / kg * sc, 2. * kr * (1. - kr) / kg * sc, 2. * (1. - kb) * sc)
    return tuple(int(math.floor(v * float(1 << s) + .5)) for v in x), s


def test_out_coefs(v9):
    assert v9.out_coefs(2, 0, 8, 8) == ((19077, 29372, 3494, 8731, 34610), 14)
    for cs in (1, 2, 3, 4, 5):
        for d in (8, 10, 12):
            for full in (0, 1):
                for o in {8, d}:
                    c, s = v9.out_coefs(cs, full, d, o)
                    assert (c, s) == _coefs(cs, full, d, o), (cs, d, full, o)
                    # every product of the conversion stays inside int32
                    ymax = (1 << d) - 1
                    cmax = 1 << (d - 1)
                    assert c[0] * ymax + max(c[1], c[2] + c[3], c[4]) * cmax + (1 << (s - 1)) < 1 << 31
    assert v9.out_coefs(1, 0, 8, 8) == v9.out_coefs(3, 0, 8, 8)
    assert v9.out_coefs(7, 1, 10, 8) == ((0, 0, 0, 0, 0), 2)
    for cs in (0, 6):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.out_coefs(cs, 0, 8, 8)
        assert e.value.code == v9.EINVAL
    for bpp, ob in ((9, 8), (10, 12), (8, 10)):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.out_coefs(2, 0, bpp, ob)
        assert e.value.code == v9.EINVAL


def test_out_layout(v9):
    w, h = 65, 33
    assert v9.out_layout("rgb24", w, h) == (6435, 195, (0, 1, 2))
    assert v9.out_layout("rgb24", w, h, pitch=208) == (208 * 33, 208, (0, 1, 2))
    assert v9.out_layout("rgbp_u8", w, h) == (3 * 65 * 33, 65, (0, 65 * 33, 2 * 65 * 33))
    assert v9.out_layout("rgbp_u8", w, h, pitch=80) == (3 * 80 * 33, 80, (0, 80 * 33, 2 * 80 * 33))
    assert v9.out_layout("rgbp_f16", w, h) == (3 * 130 * 33, 130, (0, 130 * 33, 2 * 130 * 33))
    # semi-planar: one pitch for Y and UV rows; 4:2:0 of 65 x 33 has 33 x 17 chroma pairs
    assert v9.out_layout("semiplanar", w, h, 8, 1, 1, pitch=80) == (80 * (33 + 17), 80, (0, 80 * 33, 80 * 33 + 1))
    assert v9.out_layout("semiplanar", w, h, 8, 1, 1) == (66 * 50, 66, (0, 66 * 33, 66 * 33 + 1))
    assert v9.out_layout("semiplanar", w, h, 10, 1, 1) == (132 * 50, 132, (0, 132 * 33, 132 * 33 + 2))
    assert v9.out_layout("semiplanar", w, h, 8, 0, 0) == (130 * 66, 130, (0, 130 * 33, 130 * 33 + 1))
    assert v9.out_layout("semiplanar", w, h, 8, 1, 0)[0] == 66 * 66          # 4:2:2: 33 chroma rows
    assert v9.out_layout("semiplanar", w, h, 8, 0, 1)[0] == 130 * 50         # 4:4:0
    assert v9.out_layout("rgb24", w, h, frame_stride=7000)[0] == 6435
    for kw in (dict(pitch=194), dict(pitch=200), dict(frame_stride=6434), dict(pitch=-16)):
        with pytest.raises(v9.Vp9HipError) as e:   # too narrow; not tight and not 16-aligned; overlapping frames
            v9.out_layout("rgb24", w, h, **kw)
        assert e.value.code == v9.EINVAL
    with pytest.raises(v9.Vp9HipError):
        v9.out_layout("rgb24", 0, h)


def test_abi_version_and_struct_tails(v9):
    import ctypes
    assert v9.ABI_VERSION == 5 and v9.lib().vp9hip_abi_version() == 5
    assert [f[0] for f in v9.SynthParams._fields_[-6:]] == ["seg", "eob_dense", "ref_mix", "mv_range", "edge_large",
                                                            "p_intra"]
    assert v9.FrameInfo._fields_[-2:] == [("colorspace", ctypes.c_int32), ("full_range", ctypes.c_int32)]
    assert v9.DecodedFrameInfo._fields_[-2:] == [("colorspace", ctypes.c_int32), ("full_range", ctypes.c_int32)]
    assert ctypes.sizeof(v9.FrameInfo) == 88 and ctypes.sizeof(v9.DecodedFrameInfo) == 40
    assert ctypes.sizeof(v9.OutDesc) == 40
