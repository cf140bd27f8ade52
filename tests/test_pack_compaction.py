"""Pack compaction on the CPU lane: once early stopping has ended enough
models, the fit goes on in a child pack of the live models. Every model
ends with the weights, optimizer state, history, ``epochs_run`` and
``best_epoch`` of the same fit without compaction; only the cost
changes.

The two arms run from one ``init_p32`` snapshot. CPU packs of different
G agree to the tolerances test_early_stopping_packed.py uses between
packs of different G (rtol 1e-5, atol 1e-8): the batched matmul may sum
in another order."""
import numpy as np
import pytest
import torch

from compaction_cases import (
    assert_history_shape, fit_arm, replay_compactions,
)
from gordo_amd.engine.pack import DensePack, LSTMPack
from gordo_amd.engine.spec import LayerSpec, ModelSpec
from test_early_stopping_packed import (
    _assert_no_marginal_decision, _datasets, dense_spec,
)

G = 5
ES = {"patience": 2, "min_delta": 0.0175}
EPOCHS_RUN = [3, 5, 3, 15, 13]
COMPACTIONS = {
    0.5: [(4, 5, 2)],
    1.0: [(2, 5, 3), (4, 3, 2), (12, 2, 1)],
}


def _dense_data():
    (zeros, s_z), (sines, s_s), (noise, s_n) = _datasets()
    noise43 = (np.random.default_rng(43).random((256, 5)) * 0.5).astype(
        "float32"
    )
    sets = [(zeros, s_z), (noise, s_n), (noise43, 10), (sines, s_s),
            ((0.7 * sines).astype("float32"), 11)]
    X = torch.tensor(np.stack([x for x, _ in sets]))
    return X, [s for _, s in sets]


_OFF = {}


def _dense_arms(shuffle, restore, ratio):
    """(off pack, off history, on pack, on history); the off arm of a
    configuration runs once and is only read."""
    X, seeds = _dense_data()
    es = dict(ES, restore_best_weights=True) if restore else ES
    spec = dense_spec()
    key = (shuffle, restore)
    if key not in _OFF:
        snapshot = DensePack(spec, G, device="cpu", seeds=seeds).store.p32
        _OFF[key] = (snapshot,) + fit_arm(
            lambda: DensePack(spec, G, device="cpu", seeds=seeds,
                              init_p32=snapshot),
            X, dict(epochs=40, batch_size=64, shuffle=shuffle,
                    early_stopping=es), None,
        )
    snapshot, off, off_hist = _OFF[key]
    on, on_hist = fit_arm(
        lambda: DensePack(spec, G, device="cpu", seeds=seeds,
                          init_p32=snapshot),
        X, dict(epochs=40, batch_size=64, shuffle=shuffle,
                early_stopping=es), ratio,
    )
    return off, off_hist, on, on_hist


def _assert_arms_agree(off, off_hist, on, on_hist, es_cfg, compactions):
    n = off.G
    assert off_hist.compactions == []
    assert on_hist.compactions == compactions
    for g in range(n):
        _assert_no_marginal_decision(
            [r[g] for r in off_hist["loss"][: off_hist.epochs_run[g]]],
            es_cfg,
        )
    assert on_hist.epochs_run == off_hist.epochs_run
    assert on_hist.best_epoch == off_hist.best_epoch
    assert set(on_hist) == set(off_hist)
    for key in off_hist:
        assert len(on_hist[key]) == len(off_hist[key])
        for g in range(n):
            for e in range(off_hist.epochs_run[g]):
                assert on_hist[key][e][g] == pytest.approx(
                    off_hist[key][e][g], rel=1e-5, abs=1e-8
                ), (key, e, g)
    assert_history_shape(off_hist, n, [])
    assert_history_shape(on_hist, n, compactions)
    # the parent is whole again
    assert on.G == n and on.store.active is None
    assert on.store.step_count == off.store.step_count
    assert all(v.shape[0] == n for v in on.store.views.values())
    for g in range(n):
        for got, want in (
            (on.state_for_model(g), off.state_for_model(g)),
            (on.optimizer_state_for_model(g),
             off.optimizer_state_for_model(g)),
        ):
            assert set(got) == set(want)
            for name in want:
                np.testing.assert_allclose(
                    got[name], want[name], rtol=1e-5, atol=1e-8,
                    err_msg=f"model {g} {name}",
                )


@pytest.mark.parametrize("ratio", [0.5, 1.0])
@pytest.mark.parametrize("shuffle,restore", [
    (False, False), (True, False), (False, True),
])
def test_dense_pack_compacts_and_ends_as_without(shuffle, restore, ratio):
    off, off_hist, on, on_hist = _dense_arms(shuffle, restore, ratio)
    assert off_hist.epochs_run == EPOCHS_RUN
    assert COMPACTIONS[ratio] == replay_compactions(EPOCHS_RUN, ratio)
    _assert_arms_agree(off, off_hist, on, on_hist, ES, COMPACTIONS[ratio])
    if restore:
        # the best weights crossed every hop: a model's weights are the
        # off arm's, which test_early_stopping_packed pins to its best
        # epoch; they differ from the last weights somewhere
        assert any(
            b + 1 < r for b, r in zip(on_hist.best_epoch, on_hist.epochs_run)
        )


def test_early_stoppers_stay_frozen_in_the_parent_bit_for_bit():
    """A model that ended before the compaction is never touched again:
    its parent slices are those of the off arm, bit for bit."""
    off, off_hist, on, _ = _dense_arms(False, False, 1.0)
    first = [g for g, r in enumerate(off_hist.epochs_run) if r == 3]
    assert first == [0, 2]
    for name in on.param_names():
        o, n = on.store._offsets[name]
        per = n // G
        for g in first:
            for buf in ("p32", "m", "v"):
                a = getattr(on.store, buf)[o + g * per : o + (g + 1) * per]
                b = getattr(off.store, buf)[o + g * per : o + (g + 1) * per]
                assert torch.equal(a, b), (name, g, buf)


def test_compaction_off_and_no_callbacks():
    X, seeds = _dense_data()
    pack = DensePack(dense_spec(), G, device="cpu", seeds=seeds)
    hist = pack.fit(X, X.clone(), epochs=2, batch_size=64, shuffle=False)
    assert hist.compactions is None and hist.best_epoch is None
    off, off_hist, _, _ = _dense_arms(False, False, 0.5)
    assert off_hist.compactions == []


def test_bad_ratio_raises_when_the_fit_starts(monkeypatch):
    X, seeds = _dense_data()
    pack = DensePack(dense_spec(), G, device="cpu", seeds=seeds)
    before = pack.store.p32.clone()
    monkeypatch.setenv("GORDO_PACK_COMPACT_RATIO", "1.5")
    with pytest.raises(ValueError):
        pack.fit(X, X.clone(), epochs=2, batch_size=64, early_stopping=ES)
    assert torch.equal(pack.store.p32, before)


def test_store_gather_and_scatter_carry_everything():
    """_ParamStore.gather_models / scatter_models: parameters, every
    slot, the extra buffer and the step counter, both ways."""
    spec = dense_spec(optimizer="Adam", optimizer_kwargs={"amsgrad": True})
    big = DensePack(spec, 4, device="cpu", seeds=[1, 2, 3, 4])
    small = DensePack(spec, 2, device="cpu", seeds=[5, 6])
    gen = torch.Generator().manual_seed(0)
    for _k, slot in big.store.slots():
        slot.copy_(torch.rand(slot.shape, generator=gen))
    assert [k for k, _ in big.store.slots()] == ["m", "v", "vhat"]
    extra_big = torch.rand(big.store.p32.shape, generator=gen)
    extra_small = torch.zeros_like(small.store.p32)
    big.store.step_count = 17
    live = [3, 1]
    big.store.gather_models(small.store, live, (extra_small, extra_big))
    assert small.store.step_count == 17
    assert torch.equal(big.store.gathered_p32(live), small.store.p32)
    for j, g in enumerate(live):
        assert torch.equal(small.store.views["W0"][j],
                           big.store.views["W0"][g])
        want = big.optimizer_state_for_model(g)
        got = small.optimizer_state_for_model(j)
        for name in want:
            assert np.array_equal(got[name], want[name]), name
    # scatter into a fresh parent: only the live models arrive
    other = DensePack(spec, 4, device="cpu", seeds=[9, 9, 9, 9])
    keep = other.store.p32.clone()
    extra_other = torch.zeros_like(other.store.p32)
    small.store.step_count = 23
    other.store.scatter_models(small.store, live, (extra_other, extra_small))
    assert other.store.step_count == 23
    for name in other.param_names():
        o, n = other.store._offsets[name]
        per = n // 4
        for g in range(4):
            sl = slice(o + g * per, o + (g + 1) * per)
            if g in live:
                assert torch.equal(other.store.p32[sl], big.store.p32[sl])
                assert torch.equal(other.store.vhat[sl], big.store.vhat[sl])
                assert torch.equal(extra_other[sl], extra_big[sl])
            else:
                assert torch.equal(other.store.p32[sl], keep[sl])
                assert not extra_other[sl].any()


def _lstm_spec():
    return ModelSpec(
        model_type="lstm", n_features=8, n_features_out=8,
        layers=[
            LayerSpec(kind="lstm", units=8, return_sequences=True),
            LayerSpec(kind="lstm", units=8, return_sequences=False),
            LayerSpec(kind="dense", units=8, activation="linear"),
        ],
        lookback_window=4,
    )


def test_lstm_pack_compacts_and_ends_as_without():
    """H = 8, F = 8, lookback 4, ratio 1.0, shuffled. Three noise sets
    of different scale stall one after the other (the largest not
    before the epoch cap), the large sines never do: the last child
    runs into the cap with three models."""
    n, f = 260, 8
    t = np.linspace(0, 12, n)
    noise = [np.random.default_rng(s).random((n, f)) * 0.5 * k
             for s, k in ((42, 1.0), (43, 1.5), (44, 2.5))]
    s1 = np.stack([np.sin(t + p) for p in np.linspace(0, 2, f)], axis=1) * 2
    s2 = np.stack(
        [np.cos(2 * t + p) for p in np.linspace(0, 3, f)], axis=1
    ) * 3
    X = torch.tensor(np.stack(noise + [s1, s2]).astype("float32"))
    es = {"monitor": "loss", "patience": 1, "min_delta": 0.01}
    seeds = [1, 2, 3, 4, 5]
    fit = dict(epochs=14, batch_size=64, shuffle=True, early_stopping=es)
    snapshot = LSTMPack(_lstm_spec(), G, device="cpu", seeds=seeds).store.p32

    def make():
        return LSTMPack(_lstm_spec(), G, device="cpu", seeds=seeds,
                        init_p32=snapshot)

    off, off_hist = fit_arm(make, X, fit, None)
    on, on_hist = fit_arm(make, X, fit, 1.0)
    assert off_hist.epochs_run == [2, 11, 14, 14, 14]
    want = [(1, 5, 4), (10, 4, 3)]
    assert want == replay_compactions(off_hist.epochs_run, 1.0)
    _assert_arms_agree(off, off_hist, on, on_hist, es, want)
