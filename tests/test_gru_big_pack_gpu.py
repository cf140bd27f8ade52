"""A wide GRU raw spec on the GPU: ``GRUPack`` on the two-step scans
against the CPU pack, the arms that run, inert pad columns, and the
estimator's fit / predict / round trip at 128 units. [GRU(128, seq),
GRU(96), Dense] on 5 tags (padded to 8), lookback 4, G = 2, B = 20. The
bounds of test_lstm_activation_gpu.py were measured at H <= 8 and are not
reused: by their rule, the bound is 2x the GPU-against-CPU deviation of
the tanh ``LSTMPack`` [LSTM(128), LSTM(96), Dense] at the same G, B, T,
seeds and data on the parent commit (MI355X; per-timestep at this grid):

    figure (``_deviation``)   LSTM, parent   bound (2x)   this GRU pack
    loss                      3.257e-4       6.514e-4     2.865e-4
    gradients                 3.092e-3       6.183e-3     2.916e-3
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops, serializer
from gordo_amd.engine.pack import GRUPack
from gordo_amd.machine.model.models import (
    KerasRawModelRegressor, _parse_raw_spec)
from test_lstm_activation_gpu import _deviation, _logical_grads

LOSS_BOUND, GRAD_BOUND = 2 * 3.256912e-04, 2 * 3.091562e-03
G, B, T, NF = 2, 20, 4, 5


def _raw(*gru):
    return {"keras.Sequential": {"layers": [
        {"keras.layers.GRU": kw} for kw in gru
    ] + [{"keras.layers.Dense": {"units": NF}}]}}


def _one_step(device):
    spec = _parse_raw_spec(
        _raw({"units": 128, "return_sequences": True}, {"units": 96}),
        {}, NF, NF, lookback_window=T)
    pack = GRUPack(spec, G=G, device=device, seeds=[1, 2])
    g = torch.Generator().manual_seed(21)
    Xw = torch.rand(G, B, T, NF, generator=g)
    Tb = torch.rand(G, B, NF, generator=g)
    loss = pack.train_batch(pack._to_compute(Xw), pack._to_compute(Tb))
    return pack, loss.float().cpu().numpy(), _logical_grads(pack)


def test_gpu_pack_step_matches_cpu_pack(monkeypatch):
    monkeypatch.delenv("GORDO_LSTM_ROWS", raising=False)
    monkeypatch.delenv("GORDO_PAD8", raising=False)
    launches, real = [], ops.gru_seq_bwd
    monkeypatch.setattr(ops, "gru_seq_bwd", lambda *a, **k: (
        real(*a, **k), launches.append(ops.last_gru_launch()))[0])
    gpu = _one_step("cuda")
    pack = gpu[0]
    assert pack.pad8 and pack.lstm_meta == [(8, 128, True), (128, 96, False)]
    # top layer first, seeded by dh_last alone; dX is a GEMM after the scan
    assert [(l["family"], l["has_dx"], l["last_only"]) for l in launches] == [
        ("gru_bwd_big", False, True), ("gru_bwd_big", False, False)]
    loss_dev, grad_dev = _deviation(gpu, _one_step("cpu"))
    print(f"wide gru gpu vs cpu: loss {loss_dev:.3e}, gradients {grad_dev:.3e}")
    assert loss_dev <= LOSS_BOUND and grad_dev <= GRAD_BOUND
    # input columns 5..7 of the bottom layer are pad: zero weights and grads
    for view in (pack.store.views["Wx0"], pack.store.gviews["Wx0"]):
        assert bool((view[:, NF:] == 0).all()) and bool((view[:, :NF] != 0).any())


def test_fit_predict_and_round_trip(tmp_path):
    X = np.random.default_rng(0).random((80, NF)).astype("float32")
    model = KerasRawModelRegressor(kind={"spec": _raw({"units": 128})},
                                   lookback_window=T, epochs=2, batch_size=32)
    model.fit(X, X)
    assert model._pack.device.type == "cuda" and isinstance(model._pack, GRUPack)
    assert ops.last_gru_launch()["family"].endswith("_big")
    out = model.predict(X)
    assert out.shape == (80 - T + 1, NF) and np.isfinite(out).all()
    serializer.dump(model, str(tmp_path))
    np.testing.assert_array_equal(serializer.load(str(tmp_path)).predict(X), out)
