"""bench.py --dump-outputs and the plain / --full split of its result line.

CPU: dump_outputs over a stand-in device (frames of a known pattern): the files' types,
shapes and size bound, the same sample positions in every call, samples and row sums that
are the frames'. GPU: one plain bench run at a cut-down C2 (key + 3 P at 1080p, 3 timed steps
so the last one runs in slot 2 of 4) whose dump must be the oracle's decode of the same
seeded frames, and whose line carries the headline fields and none of the --full legs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _FakeDev:
    """download(b): padded planes whose visible samples depend on (buffer, plane, row, column)."""

    def __init__(self, v9, w, h, bpp):
        self.v9, self.w, self.h, self.bpp = v9, w, h, bpp

    def download(self, b):
        planes = self.v9.alloc_planes(self.w, self.h, self.bpp)
        for p, pl in enumerate(planes):
            y, x = np.indices(pl.shape)
            pl[:] = (b * 7 + p * 3 + y * 5 + x) % (1 << self.bpp)
        return planes


def _expected_rows(v9, dev, bufs, w, h):
    return np.array([np.concatenate([p.sum(axis=1, dtype=np.int64) for p in v9.visible(dev.download(b), w, h)])
                     for b in bufs], dtype=np.float64)


@pytest.mark.parametrize("w,h,bpp", [(200, 130, 8), (129, 67, 10)])
def test_dump_outputs_files(v9, tmp_path, w, h, bpp):
    dev = _FakeDev(v9, w, h, bpp)
    bufs = [5, 6, 7]
    geom = (w, h, bpp, 0, 1)
    got = bench.dump_outputs(v9, dev, str(tmp_path / "a"), bufs, geom)
    again = bench.dump_outputs(v9, dev, str(tmp_path / "b"), bufs, geom)
    assert got == again and sorted(got) == ["row_sums.npy", "samples.npy"]
    s, r = np.load(tmp_path / "a" / "samples.npy"), np.load(tmp_path / "a" / "row_sums.npy")
    assert s.dtype == np.float32 and r.dtype == np.float64
    assert s.shape == (3, 6 * bench.DUMP_SAMPLES) and r.shape == (3, h + 2 * ((h + 1) // 2))
    assert np.array_equal(s, np.load(tmp_path / "b" / "samples.npy"))      # the same positions every run
    assert np.array_equal(r, _expected_rows(v9, dev, bufs, w, h))
    # the samples are samples of the visible planes, luma first: all within the pattern's range,
    # and each frame's differ (the pattern depends on the buffer)
    assert s.min() >= 0 and s.max() < (1 << bpp) and np.array_equal(s, np.round(s))
    assert not np.array_equal(s[0], s[1])
    k = bench.DUMP_SAMPLES
    rng = np.random.default_rng([bench.DUMP_SEED, 1])
    luma = v9.visible(dev.download(6), w, h)[0]
    ys, xs = rng.integers(0, h, 4 * k), rng.integers(0, w, 4 * k)
    assert np.array_equal(s[1, :4 * k], luma[ys, xs].astype(np.float32))


def test_dump_outputs_stays_under_its_bound(v9, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 40000)      # forces fewer samples per frame
    dev = _FakeDev(v9, 64, 64, 8)
    bench.dump_outputs(v9, dev, str(tmp_path), list(range(10)), (64, 64, 8, 0, 1))
    total = sum(np.load(tmp_path / f).nbytes for f in ("samples.npy", "row_sums.npy"))
    assert total <= 40000
    assert np.load(tmp_path / "samples.npy").shape[1] % 6 == 0


@pytest.mark.gpu
def test_plain_bench_line_and_dump(v9, orc, tmp_path):
    n, steps = 4, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C2", "--frames", str(n),
           "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["steps"] == steps and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(n * 1000.0 / d["ms_per_step"], rel=1e-3)
    for key in ("roofline", "cpu_baseline", "verify", "host_entropy", "e2e_decoder"):
        assert key not in d                      # these take runs of their own: --full
    # the dump is the decode of the seeded frames
    frames, refs, geom = bench.make_frames(v9, "C2", n)
    W, H = geom[:2]
    s, rows = np.load(tmp_path / "samples.npy"), np.load(tmp_path / "row_sums.npy")
    assert s.shape == (n, 6 * bench.DUMP_SAMPLES) and rows.shape == (n, H + 2 * ((H + 1) // 2))
    k = bench.DUMP_SAMPLES
    for i, ref in bench.oracle_frames(v9, orc, frames, refs, geom):
        planes = v9.visible(ref, W, H)
        assert np.array_equal(rows[i], np.concatenate([p.sum(axis=1, dtype=np.int64) for p in planes])), i
        rng = np.random.default_rng([bench.DUMP_SEED, i])
        want = []
        for p, cnt in zip(planes, (4 * k, k, k)):
            ys, xs = rng.integers(0, p.shape[0], cnt), rng.integers(0, p.shape[1], cnt)
            want.append(p[ys, xs])
        assert np.array_equal(s[i], np.concatenate(want).astype(np.float32)), i
