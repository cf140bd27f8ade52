"""Per-model early stopping in packed fits (CPU lane): every model of a
pack stops where its solo fit stops, keeps the weights of that fit, and
``restore_best_weights`` goes back to the best epoch's weights."""
import dataclasses

import numpy as np
import pytest
import torch

from gordo_amd.engine.pack import DensePack
from gordo_amd.engine.spec import LayerSpec, ModelSpec


def dense_spec(n_features=5, units=(4, 3, 4), **kwargs):
    layers = [
        LayerSpec(kind="dense", units=u, activation="tanh",
                  l1_activity=(1e-4 if i == 1 else 0.0))
        for i, u in enumerate(units)
    ]
    layers.append(LayerSpec(kind="dense", units=n_features, activation="linear"))
    return ModelSpec(
        model_type="feedforward", n_features=n_features,
        n_features_out=n_features, layers=layers, **kwargs,
    )


def _datasets():
    """The two data sets of test_early_stopping_group_semantics_and_drift
    (a constant zero target, which stalls at once; sines, which keep
    improving) and uniform noise, which stalls in between."""
    zeros = np.zeros((256, 5), dtype="float32")
    t = np.linspace(0, 12, 256)
    sines = np.stack(
        [np.sin(t + p) for p in np.linspace(0, 2, 5)], axis=1
    ).astype("float32")
    noise = (np.random.default_rng(42).random((256, 5)) * 0.5).astype(
        "float32"
    )
    return [(zeros, 7), (sines, 8), (noise, 9)]


def _assert_no_marginal_decision(losses, cfg):
    """Replay the rule over one solo loss curve; no comparison may lie
    within 1e-3 relative of its threshold ``best - min_delta``, or a
    last-bit difference between the packed and the solo run could flip
    a decision."""
    md, best = cfg["min_delta"], np.inf
    for e, v in enumerate(losses):
        if np.isfinite(best):
            thr = best - md
            assert abs(v - thr) > 1e-3 * abs(thr), (
                f"marginal early-stopping decision at epoch {e}: "
                f"value {v!r} against threshold {thr!r}"
            )
        if v + md < best:
            best = v


@pytest.mark.parametrize("members", [(0, 1), (0, 1, 2), (1, 2)])
def test_packed_models_stop_where_their_solo_fits_stop(members):
    spec = dense_spec()
    # min_delta: the sines' loss falls by ever smaller steps, so every
    # min_delta meets some epoch whose step is close to it; 0.0175 is a
    # value for which no decision of these curves is marginal (asserted
    # below), and the zero-target model (loss exactly 0) is not a tie
    es = {"patience": 2, "min_delta": 0.0175}
    fit = dict(epochs=40, batch_size=64, shuffle=False, early_stopping=es)
    data = [_datasets()[i] for i in members]

    solos, solo_hist = [], []
    for X, seed in data:
        solo = DensePack(spec, G=1, device="cpu", seeds=[seed])
        hist = solo.fit(torch.tensor(X[None]), torch.tensor(X[None]), **fit)
        _assert_no_marginal_decision([r[0] for r in hist["loss"]], es)
        assert hist.epochs_run == [len(hist["loss"])]
        solos.append(solo)
        solo_hist.append(hist)
    solo_len = [len(h["loss"]) for h in solo_hist]
    assert len(set(solo_len)) == len(members)  # they do stop apart
    assert max(solo_len) < 40                  # and by patience

    G = len(members)
    pack = DensePack(spec, G=G, device="cpu", seeds=[s for _, s in data])
    Xp = torch.tensor(np.stack([X for X, _ in data]))
    hist = pack.fit(Xp, Xp.clone(), **fit)

    assert hist.epochs_run == solo_len
    assert len(hist["loss"]) == max(solo_len)  # rectangular, slowest model
    assert all(len(row) == G for row in hist["loss"])
    assert pack.store.active is None           # the mask ends with the fit
    for g in range(G):
        for e in range(solo_len[g]):
            assert hist["loss"][e][g] == pytest.approx(
                solo_hist[g]["loss"][e][0], rel=1e-5, abs=1e-8
            )
        # every model ends with the weights of its solo fit, the early
        # stoppers too: they were left out of the later steps
        packed, alone = pack.state_for_model(g), solos[g].state_for_model(0)
        for name in alone:
            np.testing.assert_allclose(
                packed[name], alone[name], rtol=1e-5, atol=1e-8,
                err_msg=f"model {g} {name}",
            )


def test_stopped_model_is_frozen_bit_for_bit():
    """After its stop a model's parameters and optimizer state do not
    move, although the pack goes on training."""
    spec = dense_spec()
    data = _datasets()[:2]
    es = {"patience": 2, "min_delta": 0.0175}
    Xp = torch.tensor(np.stack([X for X, _ in data]))

    def fit(epochs):
        pack = DensePack(spec, G=2, device="cpu", seeds=[7, 8])
        hist = pack.fit(Xp, Xp.clone(), epochs=epochs, batch_size=64,
                        shuffle=False, early_stopping=es)
        return pack, hist

    long_pack, long_hist = fit(12)
    stop = long_hist.epochs_run[0]
    assert stop < 12 and long_hist.epochs_run[1] == 12
    short_pack, _ = fit(stop)
    for name in long_pack.param_names():
        off, n = long_pack.store._offsets[name]
        per = n // 2
        for buf in ("p32", "m", "v"):
            a = getattr(long_pack.store, buf)[off : off + per]
            b = getattr(short_pack.store, buf)[off : off + per]
            assert torch.equal(a, b), (name, buf)


@pytest.mark.parametrize("lr", [2.0, 1.0])
def test_restore_best_weights_matches_a_fit_of_best_epoch_plus_one(lr):
    """SGD with a learning rate at which the loss rises again: the
    final weights are those after the best epoch, bit for bit. At
    lr=2.0 the loss rises right after epoch 0; at lr=1.0 the two models
    have different best epochs and stop at different epochs."""
    spec = dense_spec(optimizer="SGD", optimizer_kwargs={"learning_rate": lr})
    (_, _), (sines, _), (noise, _) = _datasets()
    Xp = torch.tensor(np.stack([sines * 3, (noise + 1.0) * 3]))
    es = {"monitor": "loss", "patience": 2, "min_delta": 0.0,
          "restore_best_weights": True}
    pack = DensePack(spec, G=2, device="cpu", seeds=[8, 9])
    hist = pack.fit(Xp, Xp.clone(), epochs=12, batch_size=64, shuffle=False,
                    early_stopping=es)
    assert max(hist.epochs_run) < 12
    if lr == 2.0:
        assert hist.best_epoch == [0, 0]
    else:
        assert hist.best_epoch[0] != hist.best_epoch[1]
    for g in range(2):
        best = hist.best_epoch[g]
        assert best + 1 < hist.epochs_run[g]  # something to go back from
        plain = DensePack(spec, G=2, device="cpu", seeds=[8, 9])
        plain.fit(Xp, Xp.clone(), epochs=best + 1, batch_size=64,
                  shuffle=False)
        for name in pack.param_names():
            assert torch.equal(
                pack.store.views[name][g], plain.store.views[name][g]
            ), (g, name)

    # without restore_best_weights the models keep their last weights
    es_plain = dict(es, restore_best_weights=False)
    last = DensePack(spec, G=2, device="cpu", seeds=[8, 9])
    hist_last = last.fit(Xp, Xp.clone(), epochs=12, batch_size=64,
                         shuffle=False, early_stopping=es_plain)
    assert hist_last.epochs_run == hist.epochs_run
    assert not torch.equal(last.store.p32, pack.store.p32)


def test_restore_best_weights_at_the_epoch_cap_and_for_one_model():
    """A model that runs into the epoch cap is restored too, and G = 1
    takes the same path (no mask is ever set for it)."""
    spec = dense_spec(optimizer="SGD", optimizer_kwargs={"learning_rate": 2.0})
    sines = _datasets()[1][0]
    X1 = torch.tensor((sines * 3)[None])
    es = {"monitor": "loss", "patience": 50, "restore_best_weights": True}
    pack = DensePack(spec, G=1, device="cpu", seeds=[8])
    hist = pack.fit(X1, X1.clone(), epochs=4, batch_size=64, shuffle=False,
                    early_stopping=es)
    assert hist.epochs_run == [4] and hist.best_epoch == [0]
    plain = DensePack(spec, G=1, device="cpu", seeds=[8])
    plain.fit(X1, X1.clone(), epochs=1, batch_size=64, shuffle=False)
    assert torch.equal(pack.store.p32, plain.store.p32)


def test_no_callbacks_leaves_the_unmasked_step():
    spec = dense_spec()
    X = torch.tensor(np.stack([d for d, _ in _datasets()[:2]]))
    pack = DensePack(spec, G=2, device="cpu", seeds=[1, 2])
    seen = []
    step = pack.store.optimizer_step
    pack.store.optimizer_step = lambda: (seen.append(pack.store.active), step())
    hist = pack.fit(X, X.clone(), epochs=2, batch_size=64, shuffle=False)
    assert seen and all(a is None for a in seen)
    assert hist.epochs_run == [2, 2] and hist.best_epoch is None
    # G = 1 with early stopping needs no mask either
    solo = DensePack(spec, G=1, device="cpu", seeds=[1])
    seen_solo = []
    step1 = solo.store.optimizer_step
    solo.store.optimizer_step = lambda: (
        seen_solo.append(solo.store.active), step1()
    )
    solo.fit(X[:1], X[:1].clone(), epochs=2, batch_size=64, shuffle=False,
             early_stopping={"patience": 1})
    assert seen_solo and all(a is None for a in seen_solo)


def test_history_slicers_cut_to_each_models_epochs():
    from gordo_amd.engine.pack import FitHistory
    from gordo_amd.machine.model.models import _history_for_model

    hist = FitHistory({"loss": [[1.0, 2.0], [0.5, 1.5], [0.25, 1.0]]})
    hist.epochs_run = [2, 3]
    assert _history_for_model(hist, 0) == {"loss": [1.0, 0.5]}
    assert _history_for_model(hist, 1) == {"loss": [2.0, 1.5, 1.0]}
    # a plain dict (no epochs_run) is sliced whole, as before
    assert _history_for_model(dict(hist), 0) == {"loss": [1.0, 0.5, 0.25]}


def test_fleet_builder_machines_keep_their_own_history(monkeypatch):
    """One constant-data machine and one sine machine in one pack: each
    machine's history has the length of its own run."""
    from gordo_amd.core.data_providers import SineWaveDataProvider
    from gordo_amd.engine.pack import BasePack
    from gordo_amd.parallel import PackedFleetBuilder
    from gordo_amd.workflow import NormalizedConfig

    sine_values = SineWaveDataProvider._tag_values

    def tag_values(self, tag, t):
        if tag.name.startswith("const"):
            return np.full(len(t), 0.5)
        return sine_values(self, tag, t)

    monkeypatch.setattr(SineWaveDataProvider, "_tag_values", tag_values)

    fits = []
    pack_fit = BasePack.fit

    def recording_fit(self, *args, **kwargs):
        hist = pack_fit(self, *args, **kwargs)
        fits.append((self.G, kwargs.get("epochs"), hist))
        return hist

    monkeypatch.setattr(BasePack, "fit", recording_fit)

    def machine(name, prefix):
        return {
            "name": name,
            "dataset": {
                "type": "SineWaveDataset",
                "tag_list": [f"{prefix}-{j}" for j in range(4)],
                "train_start_date": "2019-01-01T00:00:00+00:00",
                "train_end_date": "2019-01-03T00:00:00+00:00",
            },
            "model": {
                "gordo_amd.machine.model.models.KerasAutoEncoder": {
                    "kind": "feedforward_hourglass",
                    "epochs": 30,
                    "callbacks": [{
                        "tensorflow.keras.callbacks.EarlyStopping": {
                            "monitor": "loss", "patience": 1,
                            "min_delta": 0.02,
                        }
                    }],
                }
            },
            "evaluation": {"cv_mode": "build_only"},
        }

    cfg = {"machines": [machine("m-const", "const"), machine("m-sine", "t")]}
    norm = NormalizedConfig(cfg, project_name="p")
    results = dict(PackedFleetBuilder(norm.machines, save_models=False)
                   .build_all())
    assert all(not isinstance(v, BaseException) for v in results.values())

    final = [h for G, _e, h in fits if G == 2]
    assert len(final) == 1  # both machines trained in one pack
    epochs_run = final[0].epochs_run
    names = [m.name for m in norm.machines]
    lengths = {}
    for name, model in results.items():
        hist = model.metadata.build_metadata.model.model_meta["history"]
        lengths[name] = len(hist["loss"])
        assert lengths[name] == epochs_run[names.index(name)]
        assert len(hist["accuracy"]) == lengths[name]
    assert lengths["m-const"] != lengths["m-sine"]
    assert len(final[0]["loss"]) == max(lengths.values())
