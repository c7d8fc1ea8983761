"""bench.py --dump-outputs (CPU side): the last timed step's gathered response records, byte for byte, as float32 .npy."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _records(n, seed=1):
    rng = np.random.default_rng(seed)
    all0 = rng.integers(0, 256, (n, 104), dtype=np.uint8)
    all1 = rng.integers(0, 256, (n, 328), dtype=np.uint8)
    return all0, all1


def test_dump_writes_every_record_exactly(tmp_path):
    all0, all1 = _records(64)
    bench.dump_outputs(types.SimpleNamespace(last_records=(all0, all1)), str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["stage0_responses.npy", "stage1_responses.npy"]
    for name, want in (("stage0_responses", all0), ("stage1_responses", all1)):
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want.astype(np.float32))


def test_dump_above_the_limit_is_a_fixed_sample_of_whole_records(tmp_path, monkeypatch):
    all0, all1 = _records(64)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 4 * (104 + 328))
    job = types.SimpleNamespace(last_records=(all0, all1))
    bench.dump_outputs(job, str(tmp_path / "a"))
    bench.dump_outputs(job, str(tmp_path / "b"))
    s0 = np.load(tmp_path / "a" / "stage0_responses.npy")
    s1 = np.load(tmp_path / "a" / "stage1_responses.npy")
    assert s0.shape == (10, 104) and s1.shape == (10, 328)
    assert s0.nbytes + s1.nbytes <= bench.DUMP_LIMIT_BYTES
    rows = [int(np.nonzero((all0 == r.astype(np.uint8)).all(axis=1))[0][0]) for r in s0]
    assert rows == sorted(rows) and len(set(rows)) == 10
    assert np.array_equal(s1, all1[rows].astype(np.float32))          # the same subcircuits in both files
    for name in ("stage0_responses", "stage1_responses"):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy")))
