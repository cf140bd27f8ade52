"""Kernel, recurrent and bias regularizers of raw model specs: parsing,
the spec layer, the oracles against torch autograd, and CPU packs
against a plain torch training loop with the penalty in the loss."""
import copy
import pickle
import re

import numpy as np
import pytest
import torch

import regularizer_cases as rc
from gordo_amd import ops
from gordo_amd.engine.pack import DensePack, LSTMPack
from gordo_amd.engine.spec import (
    LayerSpec,
    ModelSpec,
    parse_weight_regularizer,
)
from gordo_amd.machine.model import KerasRawModelRegressor
from gordo_amd.ops import reference as ref


def _raw(layers, **kwargs):
    return KerasRawModelRegressor(
        kind={"spec": {"Sequential": {"layers": layers}}}, **kwargs
    )


# ---- parsing ------------------------------------------------------------
@pytest.mark.parametrize("definition,want", rc.ACCEPTED,
                         ids=[repr(d) for d, _ in rc.ACCEPTED])
def test_accepted_regularizer_forms(definition, want):
    assert parse_weight_regularizer(definition) == want
    # and through a raw spec, on each of the three settings
    spec = _raw([
        {"LSTM": {"units": 4, "kernel_regularizer": definition,
                  "recurrent_regularizer": definition,
                  "bias_regularizer": definition}},
        {"Dense": {"units": 3, "kernel_regularizer": definition,
                   "bias_regularizer": definition}},
    ]).build_pack_spec(3)
    lstm, dense = spec.layers
    assert (lstm.kernel_l1, lstm.kernel_l2) == want
    assert (lstm.recurrent_l1, lstm.recurrent_l2) == want
    assert (lstm.bias_l1, lstm.bias_l2) == want
    assert (dense.kernel_l1, dense.kernel_l2) == want
    assert (dense.bias_l1, dense.bias_l2) == want
    assert (dense.recurrent_l1, dense.recurrent_l2) == (0.0, 0.0)


@pytest.mark.parametrize("definition,offender", rc.REJECTED,
                         ids=[repr(d) for d, _ in rc.REJECTED])
@pytest.mark.parametrize("key", ["kernel_regularizer", "bias_regularizer"])
def test_rejected_regularizer_forms_name_the_offender(definition, offender,
                                                      key):
    with pytest.raises(ValueError, match=re.escape(offender)):
        parse_weight_regularizer(definition)
    # when the spec is built, naming the setting too
    with pytest.raises(ValueError, match=re.escape(offender)) as err:
        _raw([{"Dense": {"units": 3, key: definition}}]).build_pack_spec(3)
    assert key in str(err.value)


def test_recurrent_regularizer_is_an_lstm_setting():
    with pytest.raises(ValueError, match="recurrent_regularizer"):
        _raw([{"Dense": {"units": 3, "recurrent_regularizer": "l2"}}]
             ).build_pack_spec(3)
    with pytest.raises(ValueError, match="recurrent"):
        LayerSpec("dense", 3, recurrent_l2=0.1)
    with pytest.raises(ValueError, match="kernel_l1"):
        LayerSpec("dense", 3, kernel_l1=-1.0)
    assert LayerSpec("lstm", 3, recurrent_l2=0.1).recurrent_l2 == 0.1


def test_activity_regularizer_parsing_is_unchanged():
    spec = _raw([
        {"Dense": {"units": 3, "activity_regularizer": {"l1": 0.3},
                   "kernel_regularizer": "l2"}},
        {"Dense": {"units": 3, "activity_regularizer": {
            "tensorflow.keras.regularizers.L1": {"l1": 0.5}}}},
    ]).build_pack_spec(3)
    assert [l.l1_activity for l in spec.layers] == [0.3, 0.5]
    assert [(l.kernel_l1, l.kernel_l2) for l in spec.layers] == [
        (0.0, 0.01), (0.0, 0.0)]


# ---- the spec layer -----------------------------------------------------
def test_reference_raw_spec_regularizes_the_middle_kernel_only():
    model = KerasRawModelRegressor(kind=rc.reference_raw_config())
    spec = model.build_pack_spec(4, 1)
    assert [l.units for l in spec.layers] == [10, 32, 1]
    assert spec.layers[1].kernel_l1 == 0.2
    for i, layer in enumerate(spec.layers):
        for name in ("kernel_l1", "kernel_l2", "bias_l1", "bias_l2",
                     "recurrent_l1", "recurrent_l2"):
            if (i, name) != (1, "kernel_l1"):
                assert getattr(layer, name) == 0.0, (i, name)
    plain = KerasRawModelRegressor(
        kind=rc.reference_raw_config(False)).build_pack_spec(4, 1)
    assert spec.arch_key() != plain.arch_key()
    assert spec.has_weight_regularizers() and \
        not plain.has_weight_regularizers()


def test_arch_key_separates_each_coefficient():
    base = rc.lstm_spec(4, 4, 3)
    keys = {base.arch_key()}
    for field in ("kernel", "recurrent", "bias"):
        for pair in ((0.1, 0.0), (0.0, 0.1)):
            keys.add(rc.lstm_spec(4, 4, 3, **{field: pair}).arch_key())
    assert len(keys) == 7
    assert rc.lstm_spec(4, 4, 3).arch_key() == base.arch_key()


def test_unregularized_dicts_are_what_they_were():
    old_layer_keys = ["kind", "units", "activation", "l1_activity",
                      "return_sequences"]
    layer = LayerSpec("dense", 4, "tanh", 0.1)
    assert list(layer.to_dict()) == old_layer_keys
    assert layer.to_dict() == dict(kind="dense", units=4, activation="tanh",
                                   l1_activity=0.1, return_sequences=True)
    spec = rc.dense_spec(regularized=False)
    d = spec.to_dict()
    assert list(d) == [
        "model_type", "n_features", "n_features_out", "layers",
        "lookback_window", "lookahead", "loss", "optimizer",
        "optimizer_kwargs",
    ]
    assert all(list(x) == old_layer_keys for x in d["layers"])
    # an old dict (no regularizer keys) loads, with zeros
    loaded = ModelSpec.from_dict(copy.deepcopy(d))
    assert loaded.arch_key() == spec.arch_key()
    assert not loaded.has_weight_regularizers()


def test_round_trips_preserve_the_coefficients():
    spec = rc.lstm_spec(4, 4, 3, kernel=(0.1, 0.0), recurrent=(0.0, 0.3),
                        bias=(0.2, 0.4))
    d = spec.to_dict()
    assert d["layers"][0]["recurrent_l2"] == 0.3
    # a layer without regularizers keeps the short dict beside one with
    assert "kernel_l1" not in d["layers"][1]
    for other in (ModelSpec.from_dict(copy.deepcopy(d)),
                  pickle.loads(pickle.dumps(spec))):
        assert other.arch_key() == spec.arch_key()
        assert other.layers[0].weight_regs() == {
            "kernel": (0.1, 0.0), "recurrent": (0.0, 0.3), "bias": (0.2, 0.4)
        }
    assert LayerSpec.from_dict(spec.layers[0].to_dict()) == spec.layers[0]


def test_layer_state_without_the_fields_loads_as_zeros():
    layer = LayerSpec.__new__(LayerSpec)
    layer.__setstate__(dict(kind="lstm", units=4, activation="tanh",
                            l1_activity=0.0, return_sequences=True))
    assert layer == LayerSpec("lstm", 4)
    assert layer.weight_regs() == {
        "kernel": (0.0, 0.0), "recurrent": (0.0, 0.0), "bias": (0.0, 0.0)
    }
    # the same through pickle: a spec whose layers lack the fields
    spec = rc.dense_spec(regularized=False)
    for l in spec.layers:
        for name in ("kernel_l1", "kernel_l2", "bias_l1", "bias_l2",
                     "recurrent_l1", "recurrent_l2"):
            del l.__dict__[name]
    old = pickle.loads(pickle.dumps(spec))
    assert old.arch_key() == rc.dense_spec(regularized=False).arch_key()


# ---- oracles against autograd -------------------------------------------
def _flat(tensors, G=1):
    """Flat buffer, segment table and views of [G, ...] tensors."""
    sizes = [t[0].numel() for t in tensors]
    offsets, total = rc.layout(sizes, G)
    flat = torch.cat([t.reshape(-1) for t in tensors])
    assert flat.numel() == total
    return flat, ref.segment_table(offsets, sizes)


def test_regularized_gradient_of_a_dense_model_is_autograd():
    gen = torch.Generator().manual_seed(5)
    shapes = [(1, 6, 5), (1, 5), (1, 5, 6), (1, 6)]
    coeffs = [(0.2, 0.05), (0.0, 0.1), (0.0, 0.0), (0.3, 0.0)]
    w = [(torch.rand(s, generator=gen, dtype=torch.float64) - 0.5)
         .requires_grad_() for s in shapes]
    x = torch.rand(7, 6, generator=gen, dtype=torch.float64)

    def data_loss():
        h = torch.tanh(x @ w[0][0] + w[1][0])
        return ((h @ w[2][0] + w[3][0] - x) ** 2).mean()

    penalty = sum(l1 * t.abs().sum() + l2 * (t ** 2).sum()
                  for t, (l1, l2) in zip(w, coeffs))
    g_data = torch.autograd.grad(data_loss(), w)
    g_total = torch.autograd.grad(data_loss() + penalty, w)
    p, table = _flat([t.detach() for t in w])
    g, _ = _flat(list(g_data))
    reg = ref.reg_table(*zip(*coeffs))
    got = ref.regularized_grad(p, g, table, reg, 1)
    want, _ = _flat(list(g_total))
    # the coefficients travel as fp32: 2^-24 relative on the term
    torch.testing.assert_close(got, want, rtol=0, atol=1e-7)
    assert not torch.equal(got, g)
    # the penalty oracle is the loss difference
    (pen64, pen32) = ref.weight_penalty_ref(p, table, reg, 1)
    assert pen64.dtype == torch.float64 and pen32.dtype == torch.float32
    torch.testing.assert_close(pen64[0], penalty.detach(), rtol=1e-7, atol=0)
    torch.testing.assert_close(pen32.double(), pen64, rtol=1e-6, atol=0)
    torch.testing.assert_close(
        ref.weight_penalty(p.float(), table, reg, 1).double(), pen64,
        rtol=1e-6, atol=0)
    # one SGD step of the oracle is p - lr * total gradient
    (p1, *_), _ = ref.reg_step_ref(
        "sgd", p, g, None, None, None,
        dict(learning_rate=0.25, momentum=0.0, nesterov=False), 1, table,
        reg, 1)
    torch.testing.assert_close(p1, p - 0.25 * want, rtol=0, atol=1e-7)


def test_regularized_gradient_of_an_lstm_is_autograd():
    gen = torch.Generator().manual_seed(6)
    F, H, T = 4, 3, 3
    shapes = dict(Wx0=(F, 4 * H), Wh0=(H, 4 * H), bl0=(4 * H,), Wd=(H, F),
                  bd=(F,))
    w = {k: (torch.rand(s, generator=gen, dtype=torch.float64) - 0.5)
         .requires_grad_() for k, s in shapes.items()}
    layer = LayerSpec("lstm", H, kernel_l1=0.2, recurrent_l2=0.3,
                      bias_l1=0.05, bias_l2=0.1)
    xw = torch.rand(5, T, F, generator=gen, dtype=torch.float64)

    def data_loss():
        return ((rc.lstm_forward(w, xw) - xw[:, -1]) ** 2).mean()

    names = list(w)
    g_data = torch.autograd.grad(data_loss(), [w[k] for k in names])
    g_total = torch.autograd.grad(
        data_loss() + rc.lstm_penalty(w, layer), [w[k] for k in names])
    regs = layer.weight_regs()
    coeffs = [regs["kernel"], regs["recurrent"], regs["bias"], (0.0, 0.0),
              (0.0, 0.0)]
    p, table = _flat([w[k].detach().unsqueeze(0) for k in names])
    g, _ = _flat([t.unsqueeze(0) for t in g_data])
    want, _ = _flat([t.unsqueeze(0) for t in g_total])
    reg = ref.reg_table(*zip(*coeffs))
    got = ref.regularized_grad(p, g, table, reg, 1)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-7)
    # each regularizer on its own tensor, all four gates of it
    changed = (got != g)
    for s, k in enumerate(names):
        seg = changed[rc.segment_index([t.numel() for t in w.values()], s, 1)]
        assert bool(seg.all()) == (k in ("Wx0", "Wh0", "bl0")), k
        assert bool(seg.any()) == (k in ("Wx0", "Wh0", "bl0")), k
    (pen64, _) = ref.weight_penalty_ref(p, table, reg, 1)
    torch.testing.assert_close(
        pen64[0], rc.lstm_penalty(w, layer).detach(), rtol=1e-7, atol=0)


def test_sign_of_zero_is_zero_and_masked_step_takes_reg():
    sizes = (4, 3)
    offsets, n = rc.layout(sizes, 2)
    table = ref.segment_table(offsets, sizes)
    reg = ref.reg_table([0.5, 0.0], [0.25, 0.0])
    p = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.5, 0.0, -0.0, 2.0,
                      1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    g = torch.zeros(n)
    got = ref.regularized_grad(p, g, table, reg, 2)
    assert got.tolist() == [0.0, 0.0, 1.0, -1.0, 0.75, 0.0, 0.0, 1.5,
                            0, 0, 0, 0, 0, 0]
    assert torch.equal(g, torch.zeros(n))  # g itself is not modified
    h = dict(learning_rate=0.5, momentum=0.0, nesterov=False)
    full, masked = p.clone(), p.clone()
    ops.optimizer_step("sgd", full, g, None, None, None, h, 1,
                       segments=table, reg=reg, G=2)
    assert full.tolist()[:8] == [0.0, -0.0, 0.5, -0.5, 0.125, 0.0, -0.0, 1.25]
    ops.optimizer_step("sgd", masked, g, None, None, None, h, 1,
                       active=torch.tensor([0, 1], dtype=torch.int32),
                       segments=table, reg=reg)
    assert torch.equal(masked[:4], p[:4]) and torch.equal(masked[4:], full[4:])
    with pytest.raises(ValueError, match="segment table"):
        ops.optimizer_step("sgd", p.clone(), g, None, None, None, h, 1,
                           reg=reg, G=2)


# ---- packs against a torch loop -----------------------------------------
def _max_diff(states, finals):
    return max(
        float(np.abs(states[g][k] - finals[g][k]).max())
        for g in range(len(finals)) for k in finals[g]
    )


def test_dense_pack_trains_the_regularized_model():
    """Fails without the feature: the pack then trains the plain
    model."""
    spec = rc.dense_spec()
    X = rc.dense_data()
    pack = DensePack(spec, rc.DENSE_G, device="cpu")
    np.testing.assert_allclose(
        pack.store.reg_table.numpy(),
        [[0, 0, 0.2, 0, 0, 0, 0, 0], [0, 0, 0.05, 0, 0, 0.1, 0, 0]],
        rtol=1e-7,
    )
    init = copy.deepcopy(pack.states_for_all_models())
    history = pack.fit(X, X, **rc.DENSE_FIT)
    got = pack.states_for_all_models()
    want, want_loss = rc.dense_torch_loop(init, X, spec, True)
    plain, plain_loss = rc.dense_torch_loop(init, X, spec, False)
    # 6 fp32 SGD steps on weights below 1: a few 2^-24 each
    assert _max_diff(got, want) < 2e-6
    np.testing.assert_allclose(history["loss"], want_loss, rtol=2e-6)
    # and the plain model is far away: 6 steps of lr * l1 = 0.01 each
    assert _max_diff(got, plain) > 2e-2
    assert np.all(np.asarray(history["loss"]) > plain_loss + 0.1)


def test_lstm_pack_trains_the_regularized_model_and_validates_with_it():
    G, F, H, T, N = 2, 4, 4, 3, 14
    spec = KerasRawModelRegressor(
        kind={
            "spec": {"Sequential": {"layers": [
                {"LSTM": {"units": H, "recurrent_regularizer": "l2"}},
                {"Dense": {"units": F}},
            ]}},
            "compile": {"optimizer": {"SGD": {"learning_rate": rc.LSTM_LR}}},
        },
        lookback_window=T,
    ).build_pack_spec(F)
    assert spec.layers[0].weight_regs()["recurrent"] == (0.0, 0.01)
    # a coefficient that bites within a few steps
    spec = rc.lstm_spec(F, H, T, recurrent=(0.0, 0.5))
    X = rc.lstm_data(G, N, F)
    pack = LSTMPack(spec, G, device="cpu")
    init = copy.deepcopy(pack.states_for_all_models())
    epochs, batch = 3, 4
    history = pack.fit(X, X, epochs=epochs, batch_size=batch, shuffle=False,
                       validation_split=0.25)
    n_all = N - T + 1
    n_train = int(n_all * 0.75)
    assert n_train == 9 and n_all == 12
    want, loss, val_loss = rc.lstm_torch_loop(
        init, X, spec, epochs, batch, n_train, True)
    plain, plain_loss, plain_val = rc.lstm_torch_loop(
        init, X, spec, epochs, batch, n_train, False)
    got = pack.states_for_all_models()
    assert _max_diff(got, want) < 2e-6
    np.testing.assert_allclose(history["loss"], loss, rtol=2e-6)
    np.testing.assert_allclose(history["val_loss"], val_loss, rtol=2e-6)
    # Wh is 4 orthogonal blocks: sum w^2 = 4 H, penalty about 0.5 * 16
    assert _max_diff(got, plain) > 2e-2
    assert np.all(np.asarray(history["val_loss"]) > plain_val + 1.0)
    assert np.all(np.asarray(history["loss"]) > plain_loss + 1.0)


def test_unregularized_cpu_pack_never_asks_for_a_penalty(monkeypatch):
    calls = []
    real = ops.weight_penalty
    monkeypatch.setattr(
        ops, "weight_penalty",
        lambda *a, **k: calls.append(1) or real(*a, **k))
    X = rc.dense_data()
    pack = DensePack(rc.dense_spec(False), rc.DENSE_G, device="cpu")
    assert pack.store.reg_table is None and not pack.store.regularized
    pack.fit(X, X, validation_split=0.25, **rc.DENSE_FIT)
    assert calls == []
    pack = DensePack(rc.dense_spec(True), rc.DENSE_G, device="cpu")
    pack.fit(X, X, validation_split=0.25, **rc.DENSE_FIT)
    # 2 train batches and one validation pass per epoch
    assert len(calls) == 3 * rc.DENSE_EPOCHS


# ---- through the estimator ----------------------------------------------
def test_raw_regressor_fits_the_reference_spec_with_its_regularizer():
    rng = np.random.default_rng(3)
    X = rng.random((64, 4)).astype("float32")
    y = rng.random((64, 1)).astype("float32")
    kernels = {}
    for regularized in (True, False):
        np.random.seed(11)  # the estimator draws its weight seed here
        model = KerasRawModelRegressor(
            kind=rc.reference_raw_config(regularized), epochs=40,
            batch_size=32, shuffle=False,
        )
        model.fit(X, y)
        out = model.predict(X)
        assert out.shape == (64, 1) and np.isfinite(out).all()
        assert np.isfinite(model.history["loss"]).all()
        kernels[regularized] = model._pack.state_for_model(0)["W1"]
        assert kernels[regularized].shape == (10, 32)
    # 80 SGD steps pull every |w| down by lr * l1 = 2e-4 each: 0.016,
    # against glorot weights of mean |w| 0.19 that the data loss barely
    # moves at lr 0.001
    shrink = np.abs(kernels[False]).mean() - np.abs(kernels[True]).mean()
    assert shrink > 0.008
