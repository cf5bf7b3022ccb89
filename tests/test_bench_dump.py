"""bench.py --dump-outputs: the sample it writes is fixed, within its byte budget, and holds what the trains compute (tensor entries
and norms against the dense tensor).  No GPU: the device handle is stood in for by host trains."""
import os

import numpy as np

import bench
import ttn_amd as T


class _HostBatch:
    """The two things dump_outputs reads from a DeviceTT: dims / batch and download(b)."""

    def __init__(self, d, r, B):
        self.dims, self.batch = (2,) * d, B
        self.trains = [T.rand_tt(self.dims, r, seed=30 + b) for b in range(B)]

    def download(self, b):
        return self.trains[b]


def _dense(y):
    v = np.ones((1, 1))
    for c in y.ttv_vec:                                     # first site = slowest index
        v = np.einsum("ia,nab->inb", v, c).reshape(-1, c.shape[2])
    return v[:, 0]


def test_dump_outputs_sample_is_fixed_and_faithful(tmp_path):
    d, r, B, budget = 10, 8, 40, 100_000
    batch = _HostBatch(d, r, B)
    seeds = [30 + b for b in range(B)]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    na = bench.dump_outputs(batch, seeds, a, budget_bytes=budget)
    nb = bench.dump_outputs(batch, seeds, b, budget_bytes=budget)
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and na == nb
    for f in files:
        x = np.load(os.path.join(a, f))
        assert x.dtype == np.float64
        assert np.array_equal(x, np.load(os.path.join(b, f)))
    cores = [f for f in files if f.startswith("cores_")]
    assert 0 < len(cores) < 32 and sum(np.load(os.path.join(a, f)).nbytes for f in cores) <= budget
    ids = np.load(os.path.join(a, "train_ids.npy")).astype(int)
    assert len(ids) == 32 and len(set(ids)) == 32 and {"cores_%06d.npy" % g for g in ids[:len(cores)]} == set(cores)
    entries, norms = np.load(os.path.join(a, "entries.npy")), np.load(os.path.join(a, "norms.npy"))
    ranks = np.load(os.path.join(a, "ranks.npy"))
    rng = np.random.default_rng(20240602)
    flat = (np.stack([rng.integers(0, 2, size=entries.shape[1]) for _ in range(d)], axis=1) * 2 ** np.arange(d - 1, -1, -1)).sum(1)
    for k, g in enumerate(ids):
        y = batch.trains[g]
        full = _dense(y)
        assert ranks[k].tolist() == y.ttv_rks
        assert np.allclose(entries[k], full[flat], rtol=1e-12, atol=1e-12 * np.abs(full).max())
        assert abs(norms[k] - np.linalg.norm(full)) <= 1e-12 * np.linalg.norm(full)
    g = int(cores[0][6:12])
    assert np.array_equal(np.load(os.path.join(a, cores[0])), np.concatenate([np.ravel(c, order="F") for c in batch.trains[g].ttv_vec]))
