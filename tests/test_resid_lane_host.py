"""The 4x4 residual kernels' lane routine on the host, block for block against the oracle.

k_resid / k_resid_dev / k_resid_multi transform a 4x4 block in one lane's registers with
resid4_tx (csrc/vp9hip_resid4.h); vp9hip_resid4_host runs the same routine on the CPU. Every
case here is one (transform, bit depth): DCT/ADST in the four txtp combinations and the
lossless WHT, at 8, 10 and 12 bits, every eob 1..16, 200 blocks per eob:

  - random coefficients over the whole range, small ones, and the extremes (+-32767 at
    8 bits, +-(2^(bpp+7)) above: every coefficient at one extreme, and random signs)
  - a single nonzero coefficient at each scan position below eob
  - the 16 coefficients handed in always carry junk from eob on (the kernels load 16
    whatever eob is and must ignore those)

The oracle adds and clips (vp9o_itxfm_add), so the comparison is clip(pred + r) for a flat
pred of 0, mid-range and the maximum, with r both as returned and saturated to int16 the way
the residual scratch holds it.
"""
import numpy as np
import pytest

PER_EOB = 200
CASES = [(0, 0), (0, 1), (0, 2), (0, 3), (4, 0)]     # (tx code, txtp)


def _coefs(rng, bpp, eob):
    """PER_EOB blocks of 16 scan-order coefficients, live below eob, junk from eob on."""
    lim = 32767 if bpp == 8 else (1 << (bpp + 7))
    n = PER_EOB
    c = np.zeros((n, 16), np.int64)
    k = n // 5
    c[:k] = rng.integers(-lim, lim + 1, (k, 16))
    c[k:2 * k] = rng.integers(-64, 65, (k, 16))
    c[2 * k:3 * k] = rng.choice([-lim, lim], (k, 16))
    c[3 * k] = lim
    c[3 * k + 1] = -lim
    c[3 * k + 2] = -lim - 1 if bpp == 8 else -lim
    c[3 * k + 3:4 * k] = rng.choice([-lim, 0, lim, 1, -1], (k - 3, 16))
    # single nonzero coefficient, every scan position below eob in turn
    for i in range(4 * k, n):
        pos = (i - 4 * k) % eob
        c[i, pos] = rng.choice([-lim, lim, 1, -1, int(rng.integers(-lim, lim + 1))])
    junk = rng.integers(-lim, lim + 1, (n, 16))
    c[:, eob:] = np.where(junk[:, eob:] == 0, 1, junk[:, eob:])
    return c


def _oracle(orc, bpp, tx, txtp, eob, dense, pred):
    """clip(pred + residual) of every dense block by the oracle: (n, 4, 4) [y][x]."""
    n = len(dense)
    pix = np.full((n, 4, 4), pred, np.uint8 if bpp == 8 else np.uint16)
    blk = np.ascontiguousarray(dense, np.int16 if bpp == 8 else np.int32)
    f = orc.lib().vp9o_itxfm_add
    p0, b0 = pix.ctypes.data, blk.ctypes.data
    ps, bs = pix.strides[0], blk.strides[0]
    for i in range(n):
        f(bpp, p0 + i * ps, 4, b0 + i * bs, eob, tx, txtp)
    return pix.astype(np.int64)


@pytest.mark.parametrize("bpp", [8, 10, 12])
@pytest.mark.parametrize("tx,txtp", CASES)
def test_lane_routine_vs_oracle(v9, orc, tx, txtp, bpp):
    rng = np.random.default_rng(0x4a4 + tx * 64 + txtp * 8 + bpp)
    scan = orc.scan(tx, txtp)
    mx = (1 << bpp) - 1
    for eob in range(1, 17):
        c = _coefs(rng, bpp, eob)
        res = v9.resid4_host(bpp, tx, txtp, np.full(len(c), eob), c).astype(np.int64)
        r = res.reshape(-1, 4, 4).transpose(0, 2, 1)            # [x][y] -> [y][x]
        dense = np.zeros((len(c), 16), np.int64)
        dense[:, scan[:eob]] = c[:, :eob]
        for pred in (0, 1 << (bpp - 1), mx):
            ref = _oracle(orc, bpp, tx, txtp, eob, dense, pred)
            for what, rr in (("as returned", r), ("saturated to int16", np.clip(r, -32768, 32767))):
                got = np.clip(pred + rr, 0, mx)
                if not np.array_equal(got, ref):
                    i = int(np.nonzero((got != ref).any(axis=(1, 2)))[0][0])
                    raise AssertionError("tx %d txtp %d %d-bit eob %d pred %d (%s): block %d differs\ncoefs %s\nhost\n%s\noracle\n%s"
                                         % (tx, txtp, bpp, eob, pred, what, i, c[i, :eob], got[i], ref[i]))


def test_rejects_bad_arguments(v9):
    c = np.zeros((1, 16), np.int16)
    for tcode, txtp, eob in ((1, 0, 1), (4, 1, 1), (0, 4, 1), (0, 0, 0), (0, 0, 17)):
        with pytest.raises(v9.Vp9HipError):
            v9.resid4_host(8, tcode, txtp, [eob], c)
