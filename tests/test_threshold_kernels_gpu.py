"""The threshold kernels (csrc/thresholds.hip: K10 trail_min_max, K11
windowed_quantile, K12 row_quantile) against the fp64 oracles of
gordo_amd.ops.reference at NaN, window and size edges, and the
detector path that strings K11 and K12 together.

Inputs are fp32 values built on the CPU (tests/threshold_cases.py);
the oracle sees the same values widened to fp64. Every comparison
first requires identical NaN positions. K10 only selects input values
and must equal the oracle exactly. K11/K12 must meet, per output,

    |got - want| <= 2^-21 * max(|s_lo|, |s_hi|)

with s_lo, s_hi the oracle's neighbouring order statistics (derivation
in threshold_cases.interp_bound), and be exact where nothing is
interpolated (q in {0, 1}, equal neighbours).
"""
import numpy as np
import pandas as pd
import pytest
import torch

import threshold_cases as tc
from gordo_amd import ops
from gordo_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def _dev(X):
    return torch.from_numpy(np.ascontiguousarray(X)).cuda()


def _same_nan(got, want, ctx):
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), (
        f"NaN positions differ {ctx} at {np.argwhere(ng != nw)[:8].tolist()}:"
        f" got {got[ng != nw][:8]}, want {want[ng != nw][:8]}"
    )
    return ~nw


def _assert_exact(got, want, names, ctx):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape, ctx)
    ok = _same_nan(got, want, ctx)
    bad = np.flatnonzero(ok & (got != want))
    assert bad.size == 0, (
        ctx, [(names[r], got[r], want[r]) for r in bad[:8]]
    )


def _assert_interp(got, want, s_lo, s_hi, q, names, ctx):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape, ctx)
    ok = _same_nan(got, want, ctx)
    bound = tc.interp_bound(s_lo, s_hi, q)
    err = np.abs(np.where(ok, got - want, 0.0))
    over = np.argwhere(ok & ~(err <= np.where(ok, bound, 0.0)))
    assert over.size == 0, (
        ctx,
        [(names[i[0]], tuple(i), got[tuple(i)], want[tuple(i)],
          err[tuple(i)], bound[tuple(i)]) for i in over[:8]],
    )


# ---------------------------------------------------------------------------
# K10
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,w", tc.K10_CASES)
def test_trail_min_max_vs_oracle(N, w):
    """R = 37 rows: planted first / last / second-trip windows, the NaN
    rows, all-negative and +-inf rows, random fill."""
    require_hip()
    names, X = tc.k10_case(N, w)
    assert X.shape == (tc.K10_R, N)
    want = ref.trail_min_max_ref(X, w)
    got = ops.trail_min_max(_dev(X), w)
    assert got.dtype == torch.float32 and got.shape == (tc.K10_R,)
    _assert_exact(got.cpu().numpy(), want, names, (N, w))
    # the planted windows are the only source of their row's result
    assert want[names.index("first_window")] >= 5
    assert want[names.index("last_window")] >= 5
    if N >= 256 + w:
        assert want[names.index("second_trip")] >= 5
    assert np.isnan(want[names.index("nan_every_w")])
    assert np.isnan(want[names.index("all_nan")])
    assert not np.isnan(want[names.index("nan_all_but_one")])
    assert want[names.index("all_neg_inf")] == -np.inf
    # the NaN sits inside the run of nines: excluded, never 9
    assert not want[names.index("planted_nan")] == 9.0


@pytest.mark.parametrize("N", tc.K10_N)
def test_trail_min_max_window_longer_than_series(N):
    require_hip()
    _, X = tc.k10_case(N, N)
    got = ops.trail_min_max(_dev(X), N + 1)
    assert got.shape == (tc.K10_R,) and torch.isnan(got).all()


@pytest.mark.parametrize("N,w", [(5, 2), (257, 6), (700, 144), (700, 700)])
def test_trail_min_max_single_row(N, w):
    """R = 1: the planted-NaN row on its own."""
    require_hip()
    X = tc.planted_nan_row(np.random.default_rng(3), N, w)[None, :]
    want = ref.trail_min_max_ref(X, w)
    got = ops.trail_min_max(_dev(X), w)
    assert got.shape == (1,)
    _assert_exact(got.cpu().numpy(), want, ["planted_nan"], (N, w))


def test_trail_min_max_transposed_view_and_fp64():
    """A non-contiguous [R, N] view of an [N, R] tensor, and fp64
    input holding the same (fp32-representable) values."""
    require_hip()
    N, w = 257, 6
    names, X = tc.k10_case(N, w)
    want = ref.trail_min_max_ref(X, w)
    view = _dev(X.T).t()
    assert view.shape == X.shape and not view.is_contiguous()
    _assert_exact(ops.trail_min_max(view, w).cpu().numpy(), want, names,
                  "transposed")
    got64 = ops.trail_min_max(_dev(X.astype(np.float64)), w)
    _assert_exact(got64.cpu().numpy(), want, names, "fp64")


def test_trail_min_max_cpu_and_device_identical():
    """The fold builder takes either path depending on where the pack
    lives: same NaN-bearing input, identical results."""
    require_hip()
    for N, w in ((257, 6), (700, 144)):
        names, X = tc.k10_case(N, w)
        cpu = ops.trail_min_max(torch.from_numpy(X), w).numpy()
        dev = ops.trail_min_max(_dev(X), w).cpu().numpy()
        _assert_exact(dev, cpu.astype(np.float64), names, (N, w))
        assert np.isnan(cpu).any() and not np.isnan(cpu).all()


# ---------------------------------------------------------------------------
# K11
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("w", tc.K11_W)
def test_windowed_quantile_vs_oracle(w):
    require_hip()
    for N in tc.k11_lengths(w):
        for q in tc.K11_Q:
            for names, X in tc.k11_case(w, N, q):
                want, s_lo, s_hi = ref.windowed_quantile_ref(
                    X, w, q, return_neighbours=True
                )
                got = ops.windowed_quantile(_dev(X), w, q)
                assert got.dtype == torch.float32
                assert got.shape == (4, N - w + 1)
                _assert_interp(got.cpu().numpy(), want, s_lo, s_hi, q,
                               names, (w, N, q))


def test_windowed_quantile_largest_window():
    """w = N = 8192: P at its limit, one output per row."""
    require_hip()
    names, X = tc.k11_big_case()
    w = X.shape[1]
    assert w == 8192
    for q in (0.5, 0.99):
        want, s_lo, s_hi = ref.windowed_quantile_ref(
            X, w, q, return_neighbours=True
        )
        got = ops.windowed_quantile(_dev(X), w, q)
        assert got.shape == (2, 1)
        _assert_interp(got.cpu().numpy(), want, s_lo, s_hi, q, names,
                       (w, q))
    assert (s_lo[1, 0], s_hi[1, 0]) == (0.0, 1.0)


def test_rejects_bad_windows_and_quantiles():
    require_hip()
    X = torch.zeros(2, 8200, device="cuda")
    with pytest.raises(RuntimeError, match="window too large"):
        ops.windowed_quantile(X, 8193, 0.5)
    with pytest.raises(RuntimeError, match="window longer than series"):
        ops.windowed_quantile(X[:, :20], 21, 0.5)
    with pytest.raises(RuntimeError, match="at least 1"):
        ops.windowed_quantile(X[:, :20], 0, 0.5)
    with pytest.raises(RuntimeError, match="at least 1"):
        ops.trail_min_max(X[:, :20], 0)
    for q in (-0.01, 1.01, float("nan")):
        with pytest.raises(RuntimeError, match="q must be"):
            ops.windowed_quantile(X[:, :20], 6, q)
        with pytest.raises(RuntimeError, match="q must be"):
            ops.row_quantile(X[:, :20], q)


# ---------------------------------------------------------------------------
# K12
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", tc.K12_N)
def test_row_quantile_vs_oracle(N):
    require_hip()
    for q in tc.K12_Q:
        names, X = tc.k12_case(N, q)
        want, s_lo, s_hi = ref.row_quantile_ref(
            X, q, return_neighbours=True
        )
        got = ops.row_quantile(_dev(X), q)
        assert got.dtype == torch.float32 and got.shape == (len(names),)
        _assert_interp(got.cpu().numpy(), want, s_lo, s_hi, q, names,
                       (N, q))
        assert np.isnan(want[names.index("all_nan")])
        assert want[names.index("one_valid")] == 0.3125


def test_row_quantile_rejects_long_rows():
    require_hip()
    with pytest.raises(RuntimeError, match="too large"):
        ops.row_quantile(torch.zeros(2, 16385, device="cuda"), 0.5)


# ---------------------------------------------------------------------------
# DiffBasedKFCVAnomalyDetector._device_threshold (K11 then K12)
# ---------------------------------------------------------------------------
MAX_LEN = 16384  # the gate in diff.py and row_quantile's limit


def _detector(window, p):
    from sklearn.preprocessing import MinMaxScaler

    from gordo_amd.machine.model.anomaly.diff import (
        DiffBasedKFCVAnomalyDetector,
    )

    return DiffBasedKFCVAnomalyDetector(
        base_estimator=MinMaxScaler(), window=window,
        smoothing_method="smm", threshold_percentile=p,
    )


def _metric(n, window, cols, seed):
    """Residual-like positive values with the leading NaN run that
    cross_validate leaves for a lookback model."""
    rng = np.random.default_rng([seed, n, window])
    m = rng.gamma(2.0, 0.5, size=(n, cols))
    m[:window + 3] = np.nan
    return m


def _threshold_bound(col):
    """2^-20 * max finite |value|: the fp32 cast of the input (2^-24)
    and two interpolations (2^-21 each)."""
    fin = np.abs(col[np.isfinite(col)])
    return 2.0 ** -20 * (fin.max() if fin.size else 0.0)


@pytest.mark.parametrize("p", [0.99, 0.5])
@pytest.mark.parametrize("window", [6, 144])
def test_device_threshold_vs_pandas(window, p):
    require_hip()
    det = _detector(window, p)
    for n in (max(window, 64), 200, MAX_LEN):
        m = _metric(n, window, 3, seed=1)
        frame = pd.DataFrame(m, columns=["a", "b", "c"])
        got = det._device_threshold(frame)
        assert got is not None, "device path fell back silently"
        assert isinstance(got, pd.Series)
        assert list(got.index) == ["a", "b", "c"] and got.name == p
        want = det._smoothing(frame).quantile(p)
        for c in frame.columns:
            assert np.isnan(got[c]) == np.isnan(want[c]), (n, c)
            if not np.isnan(want[c]):
                assert abs(got[c] - want[c]) <= _threshold_bound(
                    frame[c].to_numpy()
                ), (n, c, got[c], want[c])

        series = pd.Series(m[:, 0])
        got1 = det._device_threshold(series)
        assert got1 is not None, "device path fell back silently"
        assert type(got1) is float
        want1 = det._smoothing(series).quantile(p)
        assert np.isnan(got1) == np.isnan(want1), n
        if not np.isnan(want1):
            assert abs(got1 - want1) <= _threshold_bound(m[:, 0]), (
                n, got1, want1)
    # every window of the shortest window-144 series holds a NaN
    if window == 144:
        assert np.isnan(det._device_threshold(
            pd.Series(_metric(144, window, 1, seed=1)[:, 0])))


def test_device_threshold_length_gate():
    require_hip()
    det = _detector(6, 0.99)
    for n in (63, MAX_LEN + 1):
        m = _metric(n, 6, 3, seed=2)
        assert det._device_threshold(pd.Series(m[:, 0])) is None
        assert det._device_threshold(pd.DataFrame(m)) is None
