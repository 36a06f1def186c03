"""bench.py --dump-outputs: dump_outputs writes the CSR of the last timed step
(whole where small, a seeded row sample of a larger batch) as float .npy
files that identify the output exactly.  CPU only: the function takes any
torch tensors."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _csr(n, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 7, n)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cols = rng.integers(0, 2652, int(off[-1])).astype(np.int32)
    return off, cols


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_batch(tmp_path):
    import bench
    off, cols = _csr(1000, 1)
    bench.dump_outputs(str(tmp_path), torch.from_numpy(off), torch.from_numpy(cols), 42)
    got = _load(tmp_path)
    assert set(got) == {"num_labels", "sample_rows", "row_offsets", "label_counts", "labels"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["num_labels"][0] == off[-1]
    assert np.array_equal(got["sample_rows"], np.arange(1000))
    assert np.array_equal(got["row_offsets"], off[:-1])
    assert np.array_equal(got["label_counts"], np.diff(off))
    assert np.array_equal(got["labels"], cols)


def test_dump_outputs_sampled_batch(tmp_path, monkeypatch):
    """A batch above the sample size: the same seeded rows every time, each
    with its own offset, count and labels; the label cap keeps whole rows."""
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ROWS", 300)
    monkeypatch.setattr(bench, "DUMP_MAX_LABELS", 500)
    off, cols = _csr(5000, 2)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), torch.from_numpy(off), torch.from_numpy(cols), 42)
    other = cols.copy()
    other[::2] += 1  # another output of the same shape: the same rows are sampled
    bench.dump_outputs(str(b), torch.from_numpy(off), torch.from_numpy(other), 42)
    ga, gb = _load(a), _load(b)
    sel = ga["sample_rows"].astype(np.int64)
    assert 0 < len(sel) <= 300 and len(np.unique(sel)) == len(sel)
    assert np.array_equal(sel, gb["sample_rows"])
    assert np.array_equal(ga["row_offsets"], off[sel])
    assert np.array_equal(ga["label_counts"], off[sel + 1] - off[sel])
    assert ga["label_counts"].sum() == len(ga["labels"]) <= 500
    assert np.array_equal(ga["labels"], np.concatenate([cols[off[r]:off[r + 1]] for r in sel]))
    assert not np.array_equal(ga["labels"], gb["labels"])
