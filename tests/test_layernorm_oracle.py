"""LayerNormalization on the CPU lane: the fp64 oracle against torch's
layer_norm and autograd, what the raw-spec parser accepts and refuses,
Dense-only specs keeping their dicts and keys, and one DensePack step of
[Dense(6, tanh), LayerNormalization, Dense(5)] against plain autograd.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gordo_amd.engine.pack import DensePack
from gordo_amd.engine.spec import LayerSpec, ModelSpec
from gordo_amd.machine.model.models import _parse_raw_spec
from gordo_amd.ops import reference as ref


def _raw(*layers):
    return {"keras.Sequential": {"layers": [
        {f"keras.layers.{name}": kw} for name, kw in layers]}}


LN_RAW = _raw(("Dense", dict(units=6, activation="tanh")),
              ("LayerNormalization", {}), ("Dense", dict(units=5)))


@pytest.mark.parametrize("G,B,Fp,real_f,center,scale", [
    (2, 5, 12, 12, True, True),
    (2, 5, 12, 12, False, True),
    (2, 5, 12, 12, True, False),
    (3, 4, 16, 11, True, True),    # garbage in the pad columns
    (1, 3, 1, 1, True, True),      # F = 1: y = beta
])
def test_oracle_matches_torch_autograd(G, B, Fp, real_f, center, scale):
    g = torch.Generator().manual_seed(Fp + real_f)
    x = torch.randn(G, B, Fp, generator=g, dtype=torch.float64) * 3 + 1
    dy = torch.randn(G, B, Fp, generator=g, dtype=torch.float64)
    gamma = torch.randn(G, Fp, generator=g, dtype=torch.float64) if scale else None
    beta = torch.randn(G, Fp, generator=g, dtype=torch.float64) if center else None
    (y, mean, rstd), _ = ref.layer_norm_fwd_ref(x, gamma, beta, real_f, 1e-3)
    (dx, dgamma, dbeta), _ = ref.layer_norm_bwd_ref(
        dy, x, mean, rstd, gamma, real_f, center)
    eps = float(torch.tensor(1e-3, dtype=torch.float32))
    tol = dict(rtol=1e-10, atol=1e-10)
    for m in range(G):
        xt = x[m, :, :real_f].clone().requires_grad_(True)
        w = gamma[m, :real_f].clone().requires_grad_(True) if scale else None
        b = beta[m, :real_f].clone().requires_grad_(True) if center else None
        want = F.layer_norm(xt, (real_f,), w, b, eps)
        want.backward(dy[m, :, :real_f])
        torch.testing.assert_close(y[m, :, :real_f], want.detach(), **tol)
        torch.testing.assert_close(dx[m, :, :real_f], xt.grad, **tol)
        if scale:
            torch.testing.assert_close(dgamma[m, :real_f], w.grad, **tol)
        if center:
            torch.testing.assert_close(dbeta[m, :real_f], b.grad, **tol)
    assert dgamma is not None or not scale
    assert dbeta is not None or not center
    for t in (y, dx, dgamma, dbeta):
        assert t is None or bool((t[..., real_f:] == 0).all())


def test_parser_accepts_layer_normalization():
    spec = _parse_raw_spec(_raw(
        ("Dense", dict(units=6, activation="tanh")),
        ("LayerNormalization", dict(axis=[-1], epsilon=1e-5, center=False,
                                    gamma_regularizer={"l2": 0.25})),
        ("Dense", dict(units=5))), {}, 5, 5)
    ln = spec.layers[1]
    assert spec.model_type == "feedforward" and spec.n_features_out == 5
    assert (ln.kind, ln.units, ln.epsilon, ln.center, ln.scale) == (
        "layernorm", 6, 1e-5, False, True)
    assert ln.weight_regs()["kernel"] == (0.0, 0.25)
    assert spec.dense_dims() == [(5, 6, "tanh", 0.0), (6, 5, "linear", 0.0)]
    assert ModelSpec.from_dict(spec.to_dict()).arch_key() == spec.arch_key()
    assert _parse_raw_spec(LN_RAW, {}, 5, 5).layers[1].epsilon == 1e-3


@pytest.mark.parametrize("layers,match", [
    ([("Dense", dict(units=6)), ("LayerNormalization", dict(axis=1))], "axis"),
    ([("Dense", dict(units=6)), ("LayerNormalization", dict(axis=[1]))],
     "axis"),
    ([("Dense", dict(units=6)),
      ("LayerNormalization", dict(rms_scaling=True))], "rms_scaling"),
    ([("Dense", dict(units=6)),
      ("LayerNormalization", dict(gamma_initializer="zeros"))],
     "gamma_initializer"),
    ([("Dense", dict(units=6)),
      ("LayerNormalization", dict(beta_constraint="non_neg"))],
     "beta_constraint"),
    ([("LayerNormalization", {})], "LayerNormalization position"),
    ([("LSTM", dict(units=6)), ("LayerNormalization", {})],
     "LayerNormalization in a LSTM stack"),
    ([("GRU", dict(units=6)), ("LayerNormalization", {})],
     "LayerNormalization in a GRU stack"),
    ([("Conv1D", dict(filters=8, kernel_size=2, padding="same")),
      ("LayerNormalization", {}), ("Flatten", {})],
     "LayerNormalization in a Conv1D stack"),
    ([("Dense", dict(units=6)), ("Dropout", dict(rate=0.1))],
     "Unsupported layer"),
])
def test_parser_refuses_by_name(layers, match):
    with pytest.raises(ValueError, match=match):
        _parse_raw_spec(_raw(*layers, ("Dense", dict(units=5))), {}, 5, 5)


def test_dense_only_spec_keeps_its_dict_and_key():
    spec = ModelSpec(
        model_type="feedforward", n_features=4, n_features_out=4,
        layers=[LayerSpec(kind="dense", units=6, activation="tanh"),
                LayerSpec(kind="dense", units=4, activation="linear",
                          kernel_l2=0.5)])
    plain = {"kind": "dense", "units": 6, "activation": "tanh",
             "l1_activity": 0.0, "return_sequences": True}
    assert spec.to_dict() == {
        "model_type": "feedforward", "n_features": 4, "n_features_out": 4,
        "layers": [plain, {
            "kind": "dense", "units": 4, "activation": "linear",
            "l1_activity": 0.0, "return_sequences": True,
            "kernel_l1": 0.0, "kernel_l2": 0.5, "bias_l1": 0.0,
            "bias_l2": 0.0, "recurrent_l1": 0.0, "recurrent_l2": 0.0}],
        "lookback_window": 1, "lookahead": 0, "loss": "mse",
        "optimizer": "Adam", "optimizer_kwargs": {}}
    assert spec.arch_key() == (
        "feedforward", 4, 4,
        (("dense", 6, "tanh", 0.0, True, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
         ("dense", 4, "linear", 0.0, True, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0)),
        1, 0, 1, "mse", (), "adam",
        (("amsgrad", False), ("beta_1", 0.9), ("beta_2", 0.999),
         ("epsilon", 1e-07), ("learning_rate", 0.001)))
    # a layer pickled before the layernorm fields existed restores
    old = LayerSpec.__new__(LayerSpec)
    old.__setstate__(dict(plain))
    assert (old.epsilon, old.center, old.scale) == (1e-3, True, True)
    assert old.to_dict() == plain


@pytest.mark.parametrize("pad8", ["1", "0"])
def test_cpu_pack_step_matches_plain_torch(monkeypatch, pad8):
    """Logical widths 5 -> 6 -> LN -> 5. Loss and gradients within the
    bound tests/test_gru_oracle.py holds the same comparison to."""
    monkeypatch.setenv("GORDO_PAD8", pad8)
    pack = DensePack(_parse_raw_spec(LN_RAW, {}, 5, 5), G=2, device="cpu",
                     seeds=[3, 4])
    assert pack.param_names() == ["W0", "b0", "ln0_gamma", "ln0_beta",
                                  "W1", "b1"]
    g = torch.Generator().manual_seed(7)
    X = torch.rand(2, 7, 5, generator=g)
    Tgt = torch.rand(2, 7, 5, generator=g)
    # gamma and beta off their initial values, so both gradients matter
    pack.store.views["ln0_gamma"].add_(torch.rand(2, 6, generator=g) - 0.5)
    pack.store.views["ln0_beta"].add_(torch.rand(2, 6, generator=g) - 0.5)
    st = {n: pack.store.views[n].clone().requires_grad_(True)
          for n in pack.param_names()}
    h = torch.tanh(torch.bmm(X, st["W0"]) + st["b0"].unsqueeze(1))
    h = F.layer_norm(h, (6,), None, None, 1e-3)
    h = h * st["ln0_gamma"].unsqueeze(1) + st["ln0_beta"].unsqueeze(1)
    y = torch.bmm(h, st["W1"]) + st["b1"].unsqueeze(1)
    want_loss = ((y - Tgt) ** 2).mean(dim=(1, 2))
    want_loss.sum().backward()
    np.testing.assert_allclose(pack.predict(X).numpy(), y.detach().numpy(),
                               rtol=1e-4, atol=1e-6)
    loss = pack.train_batch(X, Tgt)
    np.testing.assert_allclose(loss.numpy(), want_loss.detach().numpy(),
                               rtol=1e-4)
    for name in pack.param_names():
        assert float(st[name].grad.abs().max()) > 0, name
        np.testing.assert_allclose(pack.store.gviews[name].numpy(),
                                   st[name].grad.numpy(), rtol=2e-3, atol=1e-5)
