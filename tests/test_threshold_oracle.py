"""The fp64 threshold oracles (reference.trail_min_max_ref,
windowed_quantile_ref, row_quantile_ref) against code they share
nothing with — pandas rolling and numpy nanquantile — on the case
tables the device tests use, plus the CPU paths around the kernels
(machine/model/utils.trail_min_max and the CPU-tensor fallbacks of
ops.trail_min_max / windowed_quantile / row_quantile).
"""
import warnings

import numpy as np
import pandas as pd
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

import threshold_cases as tc
from gordo_amd import ops
from gordo_amd.machine.model.utils import trail_min_max
from gordo_amd.ops import reference as ref

TOL = 1e-12


def _close(got, want, names=None, tol=TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    assert got.shape == want.shape
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), (names, got, want)
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol,
                               err_msg=str(names))


def _pandas_tmm(X64, w):
    return pd.DataFrame(X64.T).rolling(w).min().max().to_numpy()


def _check_tmm_oracle(names, X, w):
    """The oracle against pandas on every row without an infinity, and
    against a strided-view max-of-min on the NaN-free rows with one.
    pandas rolling turns +-inf into missing values before it computes;
    the kernels and the oracle treat them as ordinary values (a row of
    -inf gives -inf)."""
    X64 = X.astype(np.float64)
    want = ref.trail_min_max_ref(X, w)
    fin = np.array(["inf" not in n for n in names])
    assert fin.sum() >= len(names) - 4
    _close(want[fin], _pandas_tmm(X64[fin], w),
           [n for n in names if "inf" not in n])
    for r in np.flatnonzero(~fin):
        view = np.lib.stride_tricks.sliding_window_view(X64[r], w)
        assert want[r] == view.min(axis=1).max(), names[r]
    if "all_neg_inf" in names:
        assert want[names.index("all_neg_inf")] == -np.inf
        assert want[names.index("pos_inf_window")] == np.inf
    return want


# ---------------------------------------------------------------------------
# the oracles vs pandas / numpy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,w", tc.K10_CASES)
def test_trail_min_max_ref_vs_pandas(N, w):
    names, X = tc.k10_case(N, w)
    _check_tmm_oracle(names, X, w)


@pytest.mark.parametrize("N", tc.K10_N)
def test_trail_min_max_ref_window_longer_than_series(N):
    _, X = tc.k10_case(N, N)
    got = ref.trail_min_max_ref(X, N + 1)
    assert got.shape == (X.shape[0],) and np.isnan(got).all()
    assert np.isnan(_pandas_tmm(X.astype(np.float64), N + 1)).all()


def test_trail_min_max_ref_issue_example():
    """pandas 2.0; a NaN-ignoring window min gives 9.0."""
    x = np.array([[1, 2, 3, 9, np.nan, 9, 9, 2, 1, 1.5, 1.2]])
    assert ref.trail_min_max_ref(x, 3)[0] == 2.0
    assert pd.Series(x[0]).rolling(3).min().max() == 2.0


def _pandas_wq(X64, w, q):
    return (
        pd.DataFrame(X64.T).rolling(w).quantile(q).to_numpy().T[:, w - 1:]
    )


@pytest.mark.parametrize("w", tc.K11_W)
def test_windowed_quantile_ref_vs_pandas(w):
    for N in tc.k11_lengths(w):
        for q in tc.K11_Q:
            for names, X in tc.k11_case(w, N, q):
                got, s_lo, s_hi = ref.windowed_quantile_ref(
                    X, w, q, return_neighbours=True
                )
                assert got.shape == (X.shape[0], N - w + 1)
                _close(got, _pandas_wq(X.astype(np.float64), w, q),
                       (names, N, q))
                ok = ~np.isnan(got)
                assert np.array_equal(np.isnan(s_lo), ~ok)
                assert (s_lo[ok] <= got[ok]).all()
                assert (got[ok] <= s_hi[ok]).all()


def test_windowed_quantile_ref_step_rows_straddle():
    """The step rows put every interior q between a 0 and a 1."""
    for w in (2, 7, 144, 1024):
        for q in (0.25, 0.99):
            names, X = tc.k11_case(w, w + 5, q)[1]
            r = names.index("step")
            _, s_lo, s_hi = ref.windowed_quantile_ref(
                X[r:r + 1], w, q, return_neighbours=True
            )
            assert (s_lo == 0).all() and (s_hi == 1).all()


def test_windowed_quantile_ref_big_window_vs_pandas():
    names, X = tc.k11_big_case()
    w = X.shape[1]
    for q in (0.5, 0.99):
        _close(ref.windowed_quantile_ref(X, w, q),
               _pandas_wq(X.astype(np.float64), w, q), names)


def test_windowed_quantile_ref_rejects_long_window():
    with pytest.raises(ValueError):
        ref.windowed_quantile_ref(np.zeros((2, 5)), 6, 0.5)


@pytest.mark.parametrize("N", tc.K12_N)
def test_row_quantile_ref_vs_nanquantile(N):
    for q in tc.K12_Q:
        names, X = tc.k12_case(N, q)
        X64 = X.astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # all-NaN row
            want = np.nanquantile(X64, q, axis=1)
        got, s_lo, s_hi = ref.row_quantile_ref(X, q, return_neighbours=True)
        _close(got, want, (names, q))
        assert np.isnan(got[names.index("all_nan")])
        assert got[names.index("one_valid")] == 0.3125
        if 0.0 < q < 1.0 and N >= 2:
            for kind in ("step", "step_with_nan"):
                r = names.index(kind)
                assert (s_lo[r], s_hi[r]) == (0.0, 1.0), (kind, q)


# ---------------------------------------------------------------------------
# CPU paths around the kernels
# ---------------------------------------------------------------------------
def test_utils_trail_min_max_issue_example():
    x = np.array([1, 2, 3, 9, np.nan, 9, 9, 2, 1, 1.5, 1.2])
    assert float(trail_min_max(x, 3)) == 2.0


@pytest.mark.parametrize("N,w", [(5, 2), (40, 6), (257, 6), (300, 144),
                                 (40, 40), (40, 1)])
def test_utils_trail_min_max_nan_rows(N, w):
    """Column-wise (axis=0) on 2-D input, and each column alone as 1-D,
    over the K10 NaN rows plus the -inf / +inf rows."""
    names, X = tc.k10_case(N, w, R=20)
    want = _check_tmm_oracle(names, X, w)
    X64 = X.astype(np.float64)
    got2d = trail_min_max(X64.T, w)
    assert got2d.shape == (X.shape[0],)
    _close(got2d, want, names, tol=0)
    for r, name in enumerate(names):
        got = trail_min_max(X64[r], w)
        assert np.ndim(got) == 0
        _close(got, want[r], name, tol=0)
    # window longer than the series
    assert np.isnan(trail_min_max(X64[0], N + 1))
    short = trail_min_max(X64.T, N + 1)
    assert short.shape == (X.shape[0],) and np.isnan(short).all()


def test_ops_trail_min_max_cpu_tensor():
    names, X = tc.k10_case(257, 6)
    got = ops.trail_min_max(torch.from_numpy(X), 6)
    assert got.dtype == torch.float32 and got.shape == (X.shape[0],)
    _close(got.numpy(), ref.trail_min_max_ref(X, 6), names, tol=0)
    # a single row keeps its [R] shape
    one = ops.trail_min_max(torch.from_numpy(X[:1]), 6)
    assert one.shape == (1,)


# the fallbacks compute in fp64 and return fp32: one rounding
FP32_ROUND = 2.0 ** -23


def test_ops_windowed_quantile_cpu_tensor():
    for w, N, q in ((7, 12, 0.25), (144, 149, 0.99), (3, 3, 0.5)):
        for names, X in tc.k11_case(w, N, q):
            got = ops.windowed_quantile(torch.from_numpy(X.copy()), w, q)
            assert got.dtype == torch.float32
            _close(got.numpy(), ref.windowed_quantile_ref(X, w, q),
                   (names, w, q), tol=FP32_ROUND)


def test_ops_row_quantile_cpu_tensor():
    for N, q in ((257, 0.95), (3, 0.5), (4177, 0.99)):
        names, X = tc.k12_case(N, q)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            got = ops.row_quantile(torch.from_numpy(X), q)
        assert got.dtype == torch.float32 and got.shape == (X.shape[0],)
        _close(got.numpy(), ref.row_quantile_ref(X, q), (names, q),
               tol=FP32_ROUND)


# ---------------------------------------------------------------------------
@settings(max_examples=60, deadline=None)
@given(
    n=st.integers(min_value=1, max_value=200),
    w=st.integers(min_value=1, max_value=50),
    data=st.integers(min_value=0, max_value=2 ** 31),
    nan_frac=st.floats(min_value=0.0, max_value=1.0),
)
def test_trail_min_max_nan_property(n, w, data, nan_frac):
    """trail_min_max == pandas rolling(w).min().max() == the oracle for
    any n, w with a random subset of 0..n entries set to NaN."""
    rng = np.random.default_rng(data)
    a = rng.normal(size=n)
    k = int(round(nan_frac * n))
    a[rng.permutation(n)[:k]] = np.nan
    got = trail_min_max(a, w)
    want = pd.Series(a).rolling(w).min().max()
    oracle = ref.trail_min_max_ref(a[None, :], w)[0]
    if np.isnan(want):
        assert np.isnan(got) and np.isnan(oracle)
    else:
        assert got == want and oracle == want
