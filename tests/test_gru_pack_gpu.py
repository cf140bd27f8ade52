"""A GRU raw spec through the engine on the GPU: the pack's gradients
against the CPU pack (reference ops), inert pad units, which scan arms
run, and fit / predict / serializer round trip of the estimator.

[GRU(6, return_sequences), GRU(5), Dense] on 5 tags, lookback 6, G = 3;
the GPU pack pads every width to 8. The bounds of the GPU-against-CPU
comparison are those of tests/test_lstm_activation_gpu.py (2x the
deviation its tanh LSTM pack shows between the devices). Observed on
the MI355X: loss 2.96e-4 (bound 1.42e-3), gradients 9.05e-3 (1.23e-2).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops, serializer
from gordo_amd.engine.pack import GRUPack
from gordo_amd.machine.model.models import (
    KerasRawModelRegressor, _parse_raw_spec)
from test_lstm_activation_gpu import (
    GRAD_BOUND, LOSS_BOUND, _deviation, _logical_grads)

G, B, T, NF = 3, 40, 6, 5
RAW = {"keras.Sequential": {"layers": [
    {"keras.layers.GRU": {"units": 6, "return_sequences": True}},
    {"keras.layers.GRU": {"units": 5}},
    {"keras.layers.Dense": {"units": NF}},
]}}


def _one_step(device):
    spec = _parse_raw_spec(RAW, {}, NF, NF, lookback_window=T)
    pack = GRUPack(spec, G=G, device=device, seeds=[1, 2, 3])
    g = torch.Generator().manual_seed(21)
    Xw = torch.rand(G, B, T, NF, generator=g)
    Tb = torch.rand(G, B, NF, generator=g)
    loss = pack.train_batch(pack._to_compute(Xw), pack._to_compute(Tb))
    return pack, loss.float().cpu().numpy(), _logical_grads(pack)


def test_gpu_pack_step_matches_cpu_pack(monkeypatch):
    assert ops.hip_available()
    monkeypatch.delenv("GORDO_LSTM_ROWS", raising=False)
    monkeypatch.delenv("GORDO_PAD8", raising=False)
    launches = []
    real = ops.gru_seq_bwd
    monkeypatch.setattr(ops, "gru_seq_bwd", lambda *a, **k: (
        real(*a, **k), launches.append(ops.last_gru_launch()))[0])
    gpu = _one_step("cuda")
    pack = gpu[0]
    assert pack.pad8 and pack.lstm_meta == [(8, 8, True), (8, 8, False)]
    # layer 1 (top) first: dX inside the scan, seeded by dh_last alone
    assert [(l["family"], l["has_dx"], l["last_only"]) for l in launches] == [
        ("gru_bwd", True, True), ("gru_bwd", False, False)]
    cpu = _one_step("cpu")
    loss_dev, grad_dev = _deviation(gpu, cpu)
    print(f"gru gpu vs cpu: loss deviation {loss_dev:.3e} (bound "
          f"{LOSS_BOUND:.3e}), gradient deviation {grad_dev:.3e} (bound "
          f"{GRAD_BOUND:.3e})")
    assert loss_dev <= LOSS_BOUND and grad_dev <= GRAD_BOUND
    n_pad = 0
    for name in pack.param_names():
        for m in range(G):
            view = pack.store.views[name][m]
            mask = torch.zeros_like(view)
            pack._insert_logical(name, mask, np.ones(
                pack.store.logical[name][1:], dtype=np.float32))
            n_pad += int((mask == 0).sum())
            assert bool((view[mask == 0] == 0).all()), name
            assert bool((pack.store.gviews[name][m][mask == 0] == 0).all())
    assert n_pad > 0


def test_unplanned_shape_raises_with_the_planners_message():
    spec = _parse_raw_spec({"keras.Sequential": {"layers": [
        {"keras.layers.GRU": {"units": 72}},
        {"keras.layers.Dense": {"units": NF}}]}}, {}, NF, NF, 4)
    with pytest.raises(ValueError, match="8 <= H <= 64"):
        GRUPack(spec, G=1, device="cuda")


def test_fit_predict_and_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    X = rng.random((80, NF)).astype("float32")
    model = KerasRawModelRegressor(kind={"spec": RAW}, lookback_window=T,
                                   epochs=2, batch_size=32)
    model.fit(X, X)
    assert model._pack.device.type == "cuda"
    assert isinstance(model._pack, GRUPack)
    out = model.predict(X)
    assert out.shape == (80 - T + 1, NF) and np.isfinite(out).all()
    serializer.dump(model, str(tmp_path))
    again = serializer.load(str(tmp_path)).predict(X)
    np.testing.assert_array_equal(again, out)
