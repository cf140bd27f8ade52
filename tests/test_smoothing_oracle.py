"""The fp64 smoothing oracle (reference.smooth_ref) against code it
shares nothing with — pandas rolling and ewm — on the case tables the
device tests use (tests/smoothing_cases.py), plus the CPU paths around
the kernels: ops.smooth on CPU tensors and the pandas smoothing of
DiffBasedAnomalyDetector.anomaly.

NaN positions must be identical. smm is exact; sma and ewma must be
within 1e-12 * S|x|, S|x| being the same smoothing of |x| (the bar of
test_threshold_oracle.py for oracle-vs-pandas).
"""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch
from sklearn.preprocessing import MinMaxScaler

import smoothing_cases as sc
from gordo_amd import ops
from gordo_amd.machine.model.anomaly.diff import DiffBasedAnomalyDetector
from gordo_amd.ops import reference as ref

TOL = 1e-12


def _pandas(X64, w, method):
    df = pd.DataFrame(X64.T)
    if method == "smm":
        sm = df.rolling(w).median()
    elif method == "sma":
        sm = df.rolling(w).mean()
    else:
        sm = df.ewm(span=w, adjust=True, ignore_na=False,
                    min_periods=0).mean()
    return sm.to_numpy().T


def _same_nan(got, want, ctx):
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), (
        f"NaN positions differ {ctx} at {np.argwhere(ng != nw)[:8].tolist()}"
    )
    return ~nw


def _check_vs_pandas(method, w, names, X, val, val_abs):
    keep = np.ones(len(names), dtype=bool)
    if method == "sma" and "outlier" in names:
        keep[names.index("outlier")] = False  # see the Fraction test
    want = _pandas(X.astype(np.float64), w, method)
    assert val.shape == want.shape == X.shape
    ok = _same_nan(val, want, (method, w, X.shape[1]))
    assert np.array_equal(np.isnan(val), np.isnan(val_abs))
    ok &= keep[:, None]
    err = np.abs(np.where(ok, val - want, 0.0))
    if method == "smm":
        bound = np.zeros_like(err)
    else:
        bound = TOL * np.where(ok, val_abs, 0.0)
    over = np.argwhere(err > bound)
    assert over.size == 0, (
        method, w, X.shape[1],
        [(names[i], j, val[i, j], want[i, j]) for i, j in over[:8]],
    )


@pytest.mark.parametrize("w", sc.WINDOWS)
@pytest.mark.parametrize("method", sc.METHODS)
def test_smooth_ref_vs_pandas(method, w):
    for N in sc.lengths(w):
        names, X = sc.case(w, N)
        assert X.shape == (sc.R, N) and X.dtype == np.float32
        val, val_abs = sc.oracle(method, w, N)
        _check_vs_pandas(method, w, names, X, val, val_abs)
        if method != "ewma":
            assert np.isnan(val[:, :w - 1]).all()
            assert np.isnan(val[names.index("nan_every_w")]).all()
            if N >= w:
                assert not np.isnan(val[names.index("nan_all_but_one")]).all()
        assert np.isnan(val[names.index("all_nan")]).all()


@pytest.mark.parametrize("method", sc.METHODS)
def test_smooth_ref_big_rows_vs_pandas(method):
    w, names, X = sc.big_case(method)
    val, val_abs = ref.smooth_ref(X, w, method)
    _check_vs_pandas(method, w, names, X, val, val_abs)
    if method == "sma":
        for w2, names2, X2 in sc.long_window_case():
            v2, a2 = ref.smooth_ref(X2, w2, "sma")
            _check_vs_pandas("sma", w2, names2, X2, v2, a2)


def test_smooth_ref_missing_values_are_inf_too():
    """+-inf are missing like NaN: same output as with NaN in their
    place, in all three methods."""
    w, N = 3, 66
    names, X = sc.case(w, N)
    for kind in ("pos_inf", "neg_inf"):
        row = X[names.index(kind)][None, :]
        as_nan = np.where(np.isinf(row), np.nan, row)
        for method in sc.METHODS:
            a, _ = ref.smooth_ref(row, w, method)
            b, _ = ref.smooth_ref(as_nan, w, method)
            assert np.array_equal(a, b, equal_nan=True), (kind, method)
            assert not np.isinf(a).any()
            # rolling: the windows over it are NaN; ewm: it is skipped
            assert np.isnan(a[:, w - 1:]).sum() == (0 if method == "ewma"
                                                    else w)


@pytest.mark.parametrize("w", sc.WINDOWS)
def test_sma_outlier_row_vs_exact_rationals(w, capsys):
    """The windows just past the 1e30 outlier hold only 1e-3 values: the
    oracle's mean of each is the exact rational mean to within the
    sma bound, which a sum carried across windows would miss by about
    1e30 * 2^-53 = 1e14. pandas' compensated running sum is recorded
    here, not asserted: pandas 2.3.3 recovers these windows exactly."""
    N = 700
    names, X = sc.case(w, N)
    r = names.index("outlier")
    x = X[r].astype(np.float64)
    val, val_abs = sc.oracle("sma", w, N)
    pandas_val = pd.Series(x).rolling(w).mean().to_numpy()
    first = sc.OUTLIER_AT + w  # first window that no longer holds it
    assert x[sc.OUTLIER_AT] == np.float64(np.float32(1e30))
    worst_pandas = 0.0
    for i in range(first, first + 8):
        win = x[i - w + 1:i + 1]
        assert win.max() < 3e-3
        exact = sum(Fraction(v) for v in win) / w
        bound = sc.sma_bound(w, val_abs[r, i])
        assert abs(Fraction(val[r, i]) - exact) <= Fraction(bound), (
            w, i, val[r, i], float(exact))
        worst_pandas = max(
            worst_pandas, float(abs(Fraction(pandas_val[i]) - exact)))
    with capsys.disabled():
        print(f"\n[sma outlier w={w}] pandas max |err| past the outlier: "
              f"{worst_pandas:.3e}")
    # windows that hold the outlier are dominated by it
    assert val[r, first - 1] > 1e29 / w


# ---------------------------------------------------------------------------
# CPU paths around the kernels
# ---------------------------------------------------------------------------
class _Det:
    """DiffBasedAnomalyDetector._smoothing on a bare (window, method)."""

    def __init__(self, window, method):
        self.window, self.smoothing_method = window, method

    smoothing = DiffBasedAnomalyDetector._smoothing


@pytest.mark.parametrize("method", sc.METHODS)
def test_ops_smooth_cpu_tensor_equals_smoothing(method):
    for w, N in ((1, 64), (3, 66), (144, 700), (65, 64)):
        names, X = sc.case(w, N)
        got = ops.smooth(torch.from_numpy(X.copy()), w, method)
        assert got.dtype == torch.float64 and got.shape == X.shape
        want = _Det(w, method).smoothing(pd.DataFrame(X.T)).to_numpy().T
        assert np.array_equal(got.numpy(), want, equal_nan=True), (w, N)


def test_smooth_rejects_bad_method_and_window():
    X = torch.zeros(2, 10)
    with pytest.raises(ValueError, match="smoothing method"):
        ops.smooth(X, 3, "median")
    with pytest.raises(ValueError, match="smoothing method"):
        ref.smooth_ref(X, 3, "median")
    for w in (0, -2):
        for method in sc.METHODS:
            with pytest.raises(ValueError, match="at least 1"):
                ops.smooth(X, w, method)
            with pytest.raises(ValueError, match="at least 1"):
                ref.smooth_ref(X, w, method)


def test_window_longer_than_series_is_all_nan():
    names, X = sc.case(65, 64)
    for method in ("smm", "sma"):
        val, val_abs = ref.smooth_ref(X, 65, method)
        assert val.shape == X.shape
        assert np.isnan(val).all() and np.isnan(val_abs).all()
        got = ops.smooth(torch.from_numpy(X.copy()), 65, method)
        assert got.shape == X.shape and torch.isnan(got).all()
    # ewma has no minimum window
    val, _ = ref.smooth_ref(X, 65, "ewma")
    assert not np.isnan(val[names.index("gamma")]).any()


@pytest.mark.parametrize("method", sc.METHODS)
def test_anomaly_cpu_path_is_pandas_smoothing(method, monkeypatch):
    """Without a GPU route (cuda reported absent) anomaly() gives the
    pandas families: smooth-* is _smoothing of the same frame's raw
    family, float64, same column order."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    rng = np.random.default_rng(5)
    n, F, window = 600, 5, 6
    cols = [f"tag-{i}" for i in range(F)]
    X = pd.DataFrame(rng.random((n, F)), columns=cols)
    y = X + rng.normal(0, 0.05, size=(n, F))
    det = DiffBasedAnomalyDetector(
        base_estimator=MinMaxScaler(), require_thresholds=False,
        window=window, smoothing_method=method,
    )
    det.fit(X, y)
    frame = det.anomaly(X, y)
    for raw, smooth in (
        ("tag-anomaly-scaled", "smooth-tag-anomaly-scaled"),
        ("total-anomaly-scaled", "smooth-total-anomaly-scaled"),
        ("tag-anomaly-unscaled", "smooth-tag-anomaly-unscaled"),
        ("total-anomaly-unscaled", "smooth-total-anomaly-unscaled"),
    ):
        # a scalar family (empty sub-level) selects as a Series
        want = pd.DataFrame(det._smoothing(frame[raw]))
        got = pd.DataFrame(frame[smooth])
        assert (got.dtypes == np.float64).all()
        if raw.startswith("tag-"):
            assert list(got.columns) == list(want.columns) == cols
        assert np.array_equal(got.to_numpy(), want.to_numpy(),
                              equal_nan=True), smooth
    tops = list(dict.fromkeys(c[0] for c in frame.columns))
    assert tops[-4:] == [
        "smooth-tag-anomaly-scaled", "smooth-total-anomaly-scaled",
        "smooth-tag-anomaly-unscaled", "smooth-total-anomaly-unscaled",
    ]
