"""`bench.py --dump-outputs DIR`: what the last timed step computed lands in DIR as float32 / float64 .npy files of at most
64 MB in all, a fixed seeded row sample when the full arrays would not fit.  Host tensors stand in for the runner's."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _runner(B, H):
    g = torch.Generator().manual_seed(0)
    return types.SimpleNamespace(tokens=torch.randint(0, 128256, (B,), generator=g),
                                 normed=torch.randn((B, H), generator=g).half(), x=torch.randn((B, H), generator=g).half())


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_the_step_outputs(tmp_path):
    r = _runner(16, 4096)
    assert bench.dump_outputs(r, str(tmp_path)) == ["hidden", "residual", "tokens"]
    got = _load(str(tmp_path))
    assert got["tokens"].dtype == np.float64 and np.array_equal(got["tokens"], r.tokens.numpy())
    for name, t in (("hidden", r.normed), ("residual", r.x)):
        assert got[name].dtype == np.float32 and np.array_equal(got[name], t.float().numpy())


def test_dump_samples_rows_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)
    r = _runner(64, 4096)
    bench.dump_outputs(r, str(tmp_path / "a"))
    bench.dump_outputs(r, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= (1 << 20) + 4 * 128
    rows = a["rows"].astype(np.int64)
    assert 0 < len(rows) < 64 and np.array_equal(rows, np.unique(rows))
    assert np.array_equal(a["hidden"], r.normed.float().numpy()[rows])
    for k in a:
        assert np.array_equal(a[k], b[k]), "the sample is fixed: %s" % k
