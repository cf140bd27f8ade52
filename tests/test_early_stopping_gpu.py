"""Per-model early stopping on the GPU: a model that stops early keeps,
bit for bit, the weights of a fit that ends where it stopped.

Batches hold at most 512 rows, so every weight-grad launch is a single
chunk (no fp32 atomics into dW) and a fit is reproducible bit for bit;
``shuffle=False`` keeps the batches the same between the fits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops
from gordo_amd.engine.pack import DensePack, LSTMPack
from gordo_amd.engine.spec import LayerSpec, ModelSpec

G = 3
ES = {"monitor": "loss", "patience": 1, "min_delta": 0.01}


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def _dense_spec(**kwargs):
    layers = [
        LayerSpec(kind="dense", units=u, activation="tanh")
        for u in (8, 4, 8)
    ]
    layers.append(LayerSpec(kind="dense", units=8, activation="linear"))
    return ModelSpec(model_type="feedforward", n_features=8,
                     n_features_out=8, layers=layers, **kwargs)


def _lstm_spec():
    # the smallest fused scan shape: H = 8, F = 8, lookback 4
    return ModelSpec(
        model_type="lstm", n_features=8, n_features_out=8,
        layers=[
            LayerSpec(kind="lstm", units=8, return_sequences=True),
            LayerSpec(kind="lstm", units=8, return_sequences=False),
            LayerSpec(kind="dense", units=8, activation="linear"),
        ],
        lookback_window=4,
    )


def _data():
    """Uniform noise (nothing to learn beyond its mean: stalls early)
    and two sets of large sines (improve by more than min_delta for
    many epochs)."""
    n, f = 260, 8
    t = np.linspace(0, 12, n)
    noise = np.random.default_rng(42).random((n, f)) * 0.5
    s1 = np.stack([np.sin(t + p) for p in np.linspace(0, 2, f)], axis=1) * 2
    s2 = np.stack(
        [np.cos(2 * t + p) for p in np.linspace(0, 3, f)], axis=1
    ) * 3
    return torch.tensor(
        np.stack([noise, s1, s2]).astype("float32"), device="cuda"
    )


def _model_slices(pack, g):
    """(p32 slice, mirror slice) of model g per declared tensor."""
    out = []
    for name in pack.param_names():
        off, n = pack.store._offsets[name]
        per = n // pack.G
        lo = off + g * per
        out.append((name, pack.store.p32[lo : lo + per],
                    pack.store.plp[lo : lo + per]))
    return out


def _assert_model_equal(a, b, g):
    for (name, pa, la), (_, pb, lb) in zip(_model_slices(a, g),
                                           _model_slices(b, g)):
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), name
        assert torch.equal(la.view(torch.int16), lb.view(torch.int16)), name


@pytest.mark.parametrize("kind,epochs,batch", [("dense", 12, 128),
                                               ("lstm", 6, 64)])
def test_early_stopper_keeps_the_weights_of_its_own_run(kind, epochs, batch):
    require_hip()

    def make(init=None):
        if kind == "dense":
            return DensePack(_dense_spec(), G=G, device="cuda",
                             seeds=[1, 2, 3], init_p32=init)
        return LSTMPack(_lstm_spec(), G=G, device="cuda", seeds=[1, 2, 3],
                        init_p32=init)

    X = _data()
    fit_a = make()
    snapshot = fit_a.store.p32.clone()
    hist = fit_a.fit(X, X.clone(), epochs=epochs, batch_size=batch,
                     shuffle=False, early_stopping=ES)
    assert fit_a.store.active is None  # the mask ends with the fit
    runs = hist.epochs_run
    print("epochs_run", runs)
    g_star = int(np.argmin(runs))
    # the earliest stopper did stop, and the pack trained on without it
    assert runs[g_star] < max(runs) and runs[g_star] < epochs, runs
    assert len(hist["loss"]) == max(runs)

    fit_b = make(snapshot)
    seen = []
    step = fit_b.store.optimizer_step
    fit_b.store.optimizer_step = lambda: (
        seen.append(fit_b.store.active), step()
    )
    fit_b.fit(X, X.clone(), epochs=runs[g_star], batch_size=batch,
              shuffle=False)
    # without callbacks the unmasked kernels run
    assert seen and all(a is None for a in seen)
    _assert_model_equal(fit_a, fit_b, g_star)
    # while the others did move on after model g_star froze
    other = int(np.argmax(runs))
    pa = _model_slices(fit_a, other)[0][1]
    pb = _model_slices(fit_b, other)[0][1]
    assert not torch.equal(pa, pb)


def test_restore_best_weights_on_gpu():
    """SGD at a learning rate where the loss rises after epoch 0: every
    model ends, bit for bit, with the weights (and mirror) of a plain
    fit of best_epoch + 1 epochs."""
    require_hip()
    spec = _dense_spec(optimizer="SGD",
                       optimizer_kwargs={"learning_rate": 3.0})
    X = _data()[1:] * 1.5
    es = {"monitor": "loss", "patience": 2, "restore_best_weights": True}
    pack = DensePack(spec, G=2, device="cuda", seeds=[8, 9])
    snapshot = pack.store.p32.clone()
    hist = pack.fit(X, X.clone(), epochs=10, batch_size=128, shuffle=False,
                    early_stopping=es)
    print("epochs_run", hist.epochs_run, "best_epoch", hist.best_epoch)
    for g in range(2):
        best = hist.best_epoch[g]
        assert best + 1 < hist.epochs_run[g]  # something to go back from
        plain = DensePack(spec, G=2, device="cuda", seeds=[8, 9],
                          init_p32=snapshot)
        plain.fit(X, X.clone(), epochs=best + 1, batch_size=128,
                  shuffle=False)
        _assert_model_equal(pack, plain, g)
