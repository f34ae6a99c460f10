"""bench.py's plain run and --dump-outputs: the plain line carries the headline fields and nothing measured besides; the dumped
result polynomials are exact, bounded in size, the same from run to run, and those of an oracle-verified step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakePoly:
    """download_limb of a [batch][limbs][N] result, computed on demand (a full-size headline output without the memory)"""

    def __init__(self, batch, n_limbs, N, salt):
        self.batch, self.n_limbs, self.N, self.salt = batch, n_limbs, N, salt

    def download_limb(self, b, limb):
        """every byte of a word in use: salt, entry and limb in the upper half (decodable), a position hash below"""
        i = np.arange(self.N, dtype=np.uint64)
        return np.uint64((self.salt << 56) | (b << 40) | (limb << 32)) | (i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)


class _FakeCtx:
    def sync(self):
        pass


def _words(a):
    """float32 [rows][N][8] bytes -> uint64 [rows][N]"""
    assert a.dtype == np.float32 and a.shape[-1] == 8 and a.min() >= 0 and a.max() <= 255
    return a.astype(np.uint8).reshape(-1).view("<u8").reshape(a.shape[:-1])


def test_dump_outputs_exact_bounded_and_repeatable(tmp_path):
    import bench
    big = [("ct0", _FakePoly(256, 12, 1 << 15, 1), 12), ("ct1", _FakePoly(256, 12, 1 << 15, 2), 12)]  # the headline's shape
    small = [("ct0", _FakePoly(2, 3, 1 << 10, 3), 2)]                                                   # fits: every row, limbs < 2
    for outs, d in ((big, tmp_path / "a"), (big, tmp_path / "b"), (small, tmp_path / "s")):
        bench.dump_outputs(_FakeCtx(), outs, str(d))
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == ["ct0.npy", "ct1.npy"]
    assert 32 << 20 < total <= 64 * 10**6
    for name, poly, n_limbs in big:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b)
        got = _words(a)
        rows = got.shape[0]
        assert 1 < rows < poly.batch * n_limbs
        # every dumped row is one (entry, limb) row of the result, word for word, in increasing order without repeats
        idx = []
        for row in got:
            e, limb = int(row[0] >> np.uint64(40)) & 0xFFFF, int(row[0] >> np.uint64(32)) & 0xFF
            assert e < poly.batch and limb < n_limbs and np.array_equal(row, poly.download_limb(e, limb))
            idx.append(e * n_limbs + limb)
        assert idx == sorted(set(idx))
    got = _words(np.load(tmp_path / "s" / "ct0.npy"))
    want = np.stack([_FakePoly(2, 3, 1 << 10, 3).download_limb(b, l) for b in range(2) for l in range(2)])
    assert np.array_equal(got, want)


def _bench(*args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HERING_FORCE_DEVICE")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                         timeout=timeout, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs_of_a_verified_step(tmp_path):
    """A plain run prints the headline fields for exactly --steps timed steps and measures nothing else; its dumped outputs equal,
    byte for byte, those of a --full run of the same arguments whose last step the oracle checked."""
    common = ["--steps", "3", "--warmup", "1", "--batch", "4"]
    plain = _bench(*common, "--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["n_gpus"] == 1
    assert plain["metric"] == "ciphertext-mul+relin ops/s" and plain["unit"] == "ctxt-mul+relin ops/s"
    assert plain["higher_is_better"] is True and plain["dtype"] == "u64" and plain["value"] > 0
    assert abs(plain["value"] * plain["ms_per_step"] * 1e-3 - 4) < 1e-6 * 4  # B ciphertexts per step of ms_per_step
    assert plain["verified"] is None
    for extra in ("roofline", "b1", "concurrent_b1", "ntt", "cpu_baseline", "other_configs"):
        assert extra not in plain, extra
    full = _bench(*common, "--full", "--no-b1", "--no-concurrent", "--no-ntt", "--no-cpu-baseline",
                  "--dump-outputs", str(tmp_path / "full"))
    assert full["verified"] is True, full["verified_detail"]
    assert full["roofline"]["kernel"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == ["ct0.npy", "ct1.npy"] == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype == np.float32 and a.shape[1:] == (1 << 15, 8) and 0 < a.shape[0] <= 4 * 12  # rows: (entry, limb) of B x L
        assert np.array_equal(a, b)
