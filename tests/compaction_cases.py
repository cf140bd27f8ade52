"""Shared by the pack compaction tests (CPU and GPU): the replay of the
compaction policy over a fit's ``epochs_run``, and the two-arm fit."""
import numpy as np
import pytest

from gordo_amd.engine.compaction import should_compact


def replay_compactions(epochs_run, ratio):
    """The ``(epoch, G_before, G_after)`` list a fit with these
    ``epochs_run`` has to report: after every epoch but the fit's last,
    the policy function sees the current pack size and the number of
    models that train on."""
    out, G_cur = [], len(epochs_run)
    for epoch in range(max(epochs_run) - 1):
        n_live = sum(1 for r in epochs_run if r > epoch + 1)
        if n_live < G_cur and should_compact(G_cur, n_live, ratio):
            out.append((epoch, G_cur, n_live))
            G_cur = n_live
    return out


def fit_arm(make_pack, X, fit_kwargs, ratio):
    """One fit of a fresh pack from ``make_pack()``; ``ratio`` None
    turns compaction off, else it is the compaction ratio."""
    pack = make_pack()
    with pytest.MonkeyPatch.context() as mp:
        if ratio is None:
            mp.setenv("GORDO_PACK_COMPACT", "0")
        else:
            mp.setenv("GORDO_PACK_COMPACT", "1")
            mp.setenv("GORDO_PACK_COMPACT_RATIO", repr(float(ratio)))
        hist = pack.fit(X, X.clone(), **fit_kwargs)
    return pack, hist


def assert_history_shape(hist, G, compactions):
    """Every row is [G] long; a model that was compacted out has NaN
    from the row after it left, and numbers before."""
    epochs_run = hist.epochs_run
    for key, rows in hist.items():
        assert all(len(r) == G for r in rows), key
        gone = np.zeros(G, dtype=bool)
        for e, r in enumerate(rows):
            r = np.asarray(r, dtype=np.float64)
            assert np.isnan(r[gone]).all(), (key, e)
            assert np.isfinite(r[~gone]).all(), (key, e)
            if any(c[0] == e for c in compactions):
                gone = np.asarray(epochs_run) <= e + 1
    assert len(hist["loss"]) == max(epochs_run)
