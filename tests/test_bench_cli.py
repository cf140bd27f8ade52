"""bench.py command line: result line, --steps, --dump-outputs, --full."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _load_bench():
    spec = importlib.util.spec_from_file_location("_bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_numeric_leaves_sorted_and_numeric_only():
    bench = _load_bench()
    out = []
    bench._numeric_leaves(
        {"b": [1, 2.5], "a": {"z": np.float32(3.0), "y": "text", "x": True},
         "c": None},
        out,
    )
    assert out == [3.0, 1.0, 2.5]


def test_dump_budget_samples_weights_with_fixed_seed():
    bench = _load_bench()
    rng = np.random.default_rng(1)
    arrays = {
        "weights_lstm": rng.random((3, 1000)).astype(np.float32),
        "weights_dense": rng.random((2, 40)).astype(np.float32),
        "cv_scores_lstm": rng.random((3, 10)),
    }
    whole = bench._fit_dump_budget(arrays, 1 << 20)
    assert all(whole[k] is arrays[k] for k in arrays)
    cap = 4000
    a = bench._fit_dump_budget(arrays, cap)
    b = bench._fit_dump_budget(arrays, cap)
    assert sum(v.nbytes for v in a.values()) <= cap
    assert a["cv_scores_lstm"] is arrays["cv_scores_lstm"]
    assert a["weights_dense"] is arrays["weights_dense"]  # fits its share
    assert a["weights_lstm"].shape == (3, (cap - 240) // 2 // 12)
    assert np.array_equal(a["weights_lstm"], b["weights_lstm"])
    # sampled columns are columns of the original, in order
    col0 = a["weights_lstm"][:, 0]
    assert any(np.array_equal(col0, arrays["weights_lstm"][:, j])
               for j in range(1000))


def test_steps_must_be_positive():
    proc = subprocess.run(
        [sys.executable, BENCH, "--steps", "0"],
        capture_output=True, text=True, timeout=120,
    )
    assert proc.returncode == 2
    assert "--steps" in proc.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_and_full(tmp_path, monkeypatch, capsys):
    """One tiny fleet (1 LSTM + 1 dense machine), 2 timed steps: the
    result line carries the contract keys, --steps sets the timed step
    count, and --dump-outputs leaves finite float arrays with one row
    per machine."""
    dump = tmp_path / "dump"
    monkeypatch.setattr(
        sys, "argv",
        [BENCH, "--gpus", "1", "--steps", "2", "--warmup", "0",
         "--machines-per-gpu", "2", "--full", "--dump-outputs", str(dump)],
    )
    _load_bench().main()
    stdout, stderr = capsys.readouterr()
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in res
    assert res["steps"] == 2
    assert res["ms_per_step"] > 0
    # value is machines/hour over exactly the timed steps
    assert res["value"] == pytest.approx(
        2 * 3600.0 * 1000.0 / res["ms_per_step"], rel=1e-9
    )
    # --full adds the per-phase ledger on stderr, not on stdout
    assert "phase_budget_s_per_step" in stderr

    files = sorted(p.name for p in dump.iterdir())
    expected = sorted(
        f"{q}_{kind}.npy"
        for q in ("weights", "loss_history", "feature_thresholds",
                  "aggregate_threshold", "cv_scores")
        for kind in ("lstm", "dense")
    )
    assert files == expected
    total = 0
    for name in files:
        a = np.load(dump / name)
        assert a.dtype in (np.float32, np.float64), name
        assert a.shape[0] == 1 and a.size > 0, name
        assert np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(dump / "feature_thresholds_lstm.npy").shape == (1, 50)
    assert np.load(dump / "loss_history_dense.npy").shape == (1, 5)
