"""The lane-per-column residual routine (8x8, 16x16, 32x32) on the host, block for block
against the oracle.

k_resid / k_resid_dev / k_resid_multi / k_plf transform these blocks with resid_wave
(csrc/vp9hip_kernels.hip): zero the nzr rows of the coefficients' bounding box, scatter the eob
scan-order coefficients 8N per round, a column pass over the nzc columns, a row pass, or the
DC-only shortcut. vp9hip_residn_host restates those passes on the CPU around the kernels' own
1-D transforms (csrc/vp9hip_residn.h) and their own nzc / nzr table. Every case here is one
(transform, txtp, bit depth), at the eobs where a pass changes shape: 1, 2, 3, 63, 64, 65,
8N - 1, 8N, 8N + 1, n - 1, n (those that exist for the size) and a seeded sample of others:

  - random coefficients over the whole range, small ones, and the extremes (+-32767 at 8 bits,
    +-(2^(bpp+7)) above: every coefficient at one extreme, and random signs)
  - a single nonzero coefficient at each scan position below eob; for 32x32 a sample of the
    positions, always with every position of row or column >= 12: the first 64 scan positions
    stay inside 12 columns by 9 rows, so those are the inputs of idct32 that no short block
    reaches
  - the n scan-order coefficients handed in always carry junk from eob on

The oracle adds and clips (vp9o_itxfm_add), so the comparison is clip(pred + r) for a flat
pred of 0, mid-range and the maximum, with r both as returned and saturated to int16 the way
the residual scratch holds it. Everything is exact.
"""
import numpy as np
import pytest

CASES = [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0)]     # (tx code, txtp)
PER_KIND = 6          # blocks of each random kind per eob
SAMPLED = 8           # eobs beside the listed ones
POS_SAMPLE = 48       # 32x32: single-coefficient positions beside the rows / columns >= 12


def _eobs(rng, N):
    n = N * N
    listed = {1, 2, 3, 63, 64, 65, 8 * N - 1, 8 * N, 8 * N + 1, n - 1, n}
    listed = {e for e in listed if 1 <= e <= n}
    return sorted(listed | {int(e) for e in rng.integers(1, n + 1, SAMPLED)})


def _positions(rng, N, scan, eob):
    """Scan indices below eob that get a block with that coefficient alone."""
    if N < 32:
        return np.arange(eob)
    far = np.nonzero((scan[:eob] // N >= 12) | (scan[:eob] % N >= 12))[0]
    return np.unique(np.concatenate([far, rng.integers(0, eob, POS_SAMPLE)]))


def _coefs(rng, bpp, eob, nn, positions):
    """Blocks of nn scan-order coefficients, live below eob, junk from eob on."""
    lim = 32767 if bpp == 8 else (1 << (bpp + 7))
    k = PER_KIND
    n = 4 * k + len(positions)
    c = np.zeros((n, nn), np.int64)
    c[:k] = rng.integers(-lim, lim + 1, (k, nn))
    c[k:2 * k] = rng.integers(-64, 65, (k, nn))
    c[2 * k:3 * k] = rng.choice([-lim, lim], (k, nn))
    c[3 * k] = lim
    c[3 * k + 1] = -lim
    c[3 * k + 2] = -lim - 1 if bpp == 8 else -lim
    c[3 * k + 3:4 * k] = rng.choice([-lim, 0, lim, 1, -1], (k - 3, nn))
    # single nonzero coefficient, the chosen scan positions in turn
    for i, pos in enumerate(positions):
        c[4 * k + i, pos] = rng.choice([-lim, lim, 1, -1, int(rng.integers(-lim, lim + 1))]) or 1
    junk = rng.integers(-lim, lim + 1, (n, nn))
    c[:, eob:] = np.where(junk[:, eob:] == 0, 1, junk[:, eob:])
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
def test_block_routine_vs_oracle(v9, orc, tx, txtp, bpp):
    rng = np.random.default_rng(0x4b5 + tx * 64 + txtp * 8 + bpp)
    N = 4 << tx
    scan = orc.scan(tx, txtp)
    mx = (1 << bpp) - 1
    eobs = _eobs(rng, N)
    assert {1, N * N - 1, N * N} <= set(eobs) and (N == 8 or {8 * N, 8 * N + 1, 65} <= set(eobs))
    for eob in eobs:
        c = _coefs(rng, bpp, eob, N * N, _positions(rng, N, scan, eob))
        res = v9.residn_host(bpp, tx, txtp, np.full(len(c), eob), c).astype(np.int64)
        r = res.reshape(-1, N, N).transpose(0, 2, 1)            # [x][y] -> [y][x]
        dense = np.zeros((len(c), N * N), np.int64)
        dense[:, scan[:eob]] = c[:, :eob]
        for pred in (0, 1 << (bpp - 1), mx):
            ref = _oracle(orc, bpp, tx, txtp, eob, dense, pred, N)
            for what, rr in (("as returned", r), ("saturated to int16", np.clip(r, -32768, 32767))):
                got = np.clip(pred + rr, 0, mx)
                if not np.array_equal(got, ref):
                    i = int(np.nonzero((got != ref).any(axis=(1, 2)))[0][0])
                    ys, xs = np.nonzero(got[i] != ref[i])
                    raise AssertionError("tx %d txtp %d %d-bit eob %d pred %d (%s): block %d differs at (x=%d, y=%d): "
                                         "host %d oracle %d\nnonzero scan-order coefficients %s"
                                         % (tx, txtp, bpp, eob, pred, what, i, xs[0], ys[0], got[i][ys[0], xs[0]],
                                            ref[i][ys[0], xs[0]],
                                            [(int(k), int(c[i, k])) for k in np.nonzero(c[i, :eob])[0][:40]]))


def test_first_64_scan_positions_leave_idct32_inputs_untouched(orc):
    """Why the blocks above are needed: the bounding boxes of the first 64 scan positions."""
    for tx, txtp, box in ((2, 0, (11, 9)), (2, 1, (15, 7)), (2, 2, (8, 13)), (3, 0, (12, 9))):
        N = 4 << tx
        s = orc.scan(tx, txtp)[:64]
        assert (int((s % N).max()) + 1, int((s // N).max()) + 1) == box


def test_rejects_bad_arguments(v9):
    c = np.zeros((1, 1024), np.int16)
    for tcode, txtp, eob in ((0, 0, 1), (4, 0, 1), (3, 1, 1), (1, 4, 1), (1, 0, 0), (1, 0, 65), (2, 0, 257), (3, 0, 1025)):
        nn = (4 << tcode) ** 2 if 1 <= tcode <= 3 else 16
        with pytest.raises(v9.Vp9HipError):
            v9.residn_host(8, tcode, txtp, [eob], c[:, :nn])
