"""bench.py --dump-outputs (what the timed path delivered, as float32 .npy files) and the argument checks of a plain run."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


class _PipelineState:
    def __init__(self, frames, faces):
        rng = np.random.default_rng(3)
        n = frames * faces
        self.h_counts = np.full(frames, faces, np.int32)
        self.h_boxes = rng.random((n, 4), dtype=np.float32)
        self.h_kps = rng.random((n, 98, 2), dtype=np.float32)
        self.h_scores = rng.random((n, 98), dtype=np.float32)


def test_dump_outputs_writes_what_the_pipeline_step_delivered(tmp_path):
    st = _PipelineState(6, 8)
    bench.dump_outputs(str(tmp_path), bench.timed_outputs(st))
    assert sorted(os.listdir(tmp_path)) == ["boxes.npy", "counts.npy", "landmarks.npy", "scores.npy"]
    for name, ref in (("counts", st.h_counts), ("boxes", st.h_boxes), ("landmarks", st.h_kps), ("scores", st.h_scores)):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, ref.astype(np.float32))


def test_dump_outputs_samples_the_same_rows_above_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20000)
    st = _PipelineState(10, 8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bench.timed_outputs(st))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 20000 + 4 * 128
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert 0 < a.shape[0] and np.array_equal(a, b)
    kps = np.load(tmp_path / "a" / "landmarks.npy")
    assert all(any(np.array_equal(r, q) for q in st.h_kps) for r in kps)        # whole rows of the step's output


def test_plain_run_argument_checks():
    for args, msg in ((["--steps", "0"], "--steps must be >= 1"),
                      (["--dump-profile", "x.json"], "only --full measures")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, r.stderr
