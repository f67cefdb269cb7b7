"""The gather of the lane-per-column residual routine on the host, at every tail length, against
the oracle.

resid_wave (csrc/vp9hip_kernels.hip) loads a lane's eight scan-order coefficients k0 + 8 * li ..
+ 7 whatever eob is and scatters those from eob on as zeros; in the coefficient arena they are
the next block's. vp9hip_residn_host restates that gather (and the passes behind it) on the
CPU. Here every block's live coefficients are followed by junk at the extremes of the
coefficient range (+-32767 at 8 bits, +-2^(bpp+7) above), so a junk coefficient that reaches
the transform changes the block grossly:

  - 8x8 at every eob in 1..64;
  - 16x16 and 32x32 at every eob = 0, 1, 7 (mod 8): with the 8x8 eobs that is every length of
    the last live lane's window (full, one coefficient, one short), in every round;
  - each txtp of 8x8 and 16x16, and 8, 10 and 12 bits.

Per eob three blocks: small coefficients (so that the flat prediction does not clip the
residual away), coefficients over the whole range, and a lone last coefficient eob - 1. The
oracle adds and clips (vp9o_itxfm_add), so the comparison is clip(pred + r) for a flat pred of
0, mid-range and the maximum. Everything is exact.
"""
import numpy as np
import pytest

CASES = [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0)]     # (tx code, txtp)


def _eobs(N):
    n = N * N
    return list(range(1, n + 1)) if N == 8 else [e for e in range(1, n + 1) if e % 8 in (0, 1, 7)]


def _blocks(rng, bpp, eob, nn):
    lim = 32767 if bpp == 8 else (1 << (bpp + 7))
    c = np.zeros((3, nn), np.int64)
    c[0, :eob] = rng.integers(-64, 65, eob)
    c[1, :eob] = rng.integers(-lim, lim + 1, eob)
    c[2, eob - 1] = rng.choice([-lim, lim, 1, -1, 37])
    c[:, eob:] = rng.choice([-lim, lim], (3, nn - eob))
    return c


def _oracle(orc, bpp, tx, txtp, eob, dense, pred, N):
    """clip(pred + residual) of every dense block by the oracle: (n, N, N) [y][x]."""
    n = len(dense)
    pix = np.full((n, N, N), pred, np.uint8 if bpp == 8 else np.uint16)
    blk = np.ascontiguousarray(dense, np.int16 if bpp == 8 else np.int32)
    f = orc.lib().vp9o_itxfm_add
    p0, b0 = pix.ctypes.data, blk.ctypes.data
    ps, bs = pix.strides[0], blk.strides[0]
    for i in range(n):
        f(bpp, p0 + i * ps, N, b0 + i * bs, eob, tx, txtp)
    return pix.astype(np.int64)


@pytest.mark.parametrize("bpp", [8, 10, 12])
@pytest.mark.parametrize("tx,txtp", CASES)
def test_gather_tails_vs_oracle(v9, orc, tx, txtp, bpp):
    rng = np.random.default_rng(0x6a7 + tx * 64 + txtp * 8 + bpp)
    N = 4 << tx
    scan = orc.scan(tx, txtp)
    mx = (1 << bpp) - 1
    eobs = _eobs(N)
    assert {e % 8 for e in eobs} >= {0, 1, 7} and eobs[0] == 1 and eobs[-1] == N * N
    assert N == 8 or any(e > 8 * N for e in eobs)
    c = np.concatenate([_blocks(rng, bpp, e, N * N) for e in eobs])
    be = np.repeat(eobs, 3)
    res = v9.residn_host(bpp, tx, txtp, be, c).astype(np.int64)
    r = res.reshape(-1, N, N).transpose(0, 2, 1)                # [x][y] -> [y][x]
    for k, eob in enumerate(eobs):
        blk = c[3 * k:3 * k + 3]
        dense = np.zeros((3, N * N), np.int64)
        dense[:, scan[:eob]] = blk[:, :eob]
        for pred in (0, 1 << (bpp - 1), mx):
            ref = _oracle(orc, bpp, tx, txtp, eob, dense, pred, N)
            got = np.clip(pred + r[3 * k:3 * k + 3], 0, mx)
            if not np.array_equal(got, ref):
                i = int(np.nonzero((got != ref).any(axis=(1, 2)))[0][0])
                ys, xs = np.nonzero(got[i] != ref[i])
                raise AssertionError("tx %d txtp %d %d-bit eob %d pred %d: block %d differs at (x=%d, y=%d): host %d oracle %d"
                                     % (tx, txtp, bpp, eob, pred, i, xs[0], ys[0], got[i][ys[0], xs[0]], ref[i][ys[0], xs[0]]))
