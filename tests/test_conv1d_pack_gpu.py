"""A Conv1D raw spec through the engine on the GPU: one train step of
the pack against the CPU pack (reference ops) on the same weights, inert
pad channels, and fit / predict / serializer round trip of the estimator.

[Conv1D(6, k 3, causal, relu), Conv1D(5, k 2, d 2, causal, tanh), Flatten,
Dense] on 5 tags, lookback 6, G = 3; the GPU pack pads every width to 8.
The bounds of the GPU-against-CPU comparison are those of
tests/test_lstm_activation_gpu.py, as in tests/test_gru_pack_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops, serializer
from gordo_amd.engine.pack import Conv1DPack
from gordo_amd.machine.model.models import (
    KerasRawModelRegressor, _parse_raw_spec)
from test_lstm_activation_gpu import (
    GRAD_BOUND, LOSS_BOUND, _deviation, _logical_grads)

G, B, T, NF = 3, 40, 6, 5
RAW = {"keras.Sequential": {"layers": [
    {"keras.layers.Conv1D": {"filters": 6, "kernel_size": 3,
                             "padding": "causal", "activation": "relu"}},
    {"keras.layers.Conv1D": {"filters": 5, "kernel_size": 2,
                             "dilation_rate": 2, "padding": "causal",
                             "activation": "tanh"}},
    {"keras.layers.Flatten": {}},
    {"keras.layers.Dense": {"units": NF}},
]}}


def _one_step(device):
    spec = _parse_raw_spec(RAW, {}, NF, NF, lookback_window=T)
    pack = Conv1DPack(spec, G=G, device=device, seeds=[1, 2, 3])
    g = torch.Generator().manual_seed(21)
    Xw = torch.rand(G, B, T, NF, generator=g)
    Tb = torch.rand(G, B, NF, generator=g)
    loss = pack.train_batch(pack._to_compute(Xw), pack._to_compute(Tb))
    return pack, loss.float().cpu().numpy(), _logical_grads(pack)


def test_gpu_pack_step_matches_cpu_pack(monkeypatch):
    assert ops.hip_available()
    monkeypatch.delenv("GORDO_PAD8", raising=False)
    launches = []
    for name in ("conv1d_fwd", "conv1d_wgrad", "conv1d_bwd_data"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, **k: (
            _real(*a, **k),
            launches.append(ops.last_conv1d_launch()["family"]))[0])
    gpu = _one_step("cuda")
    pack = gpu[0]
    assert pack.pad8 and [m[:4] for m in pack.conv_meta] == [
        (8, 8, 3, 1), (8, 8, 2, 2)]
    # bwd-data for the top layer only: the bottom one needs no dX
    assert launches == ["conv1d_fwd", "conv1d_fwd", "conv1d_wgrad",
                        "conv1d_bwd_data", "conv1d_wgrad"]
    cpu = _one_step("cpu")
    loss_dev, grad_dev = _deviation(gpu, cpu)
    print(f"conv1d gpu vs cpu: loss deviation {loss_dev:.3e} (bound "
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
        {"keras.layers.Conv1D": {"filters": 8, "kernel_size": 9,
                                 "padding": "same"}},
        {"keras.layers.Flatten": {}},
        {"keras.layers.Dense": {"units": NF}}]}}, {}, NF, NF, 4)
    with pytest.raises(ValueError, match="kernel_size <= 8"):
        Conv1DPack(spec, G=1, device="cuda")


def test_fit_predict_and_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    X = rng.random((80, NF)).astype("float32")
    model = KerasRawModelRegressor(kind={"spec": RAW}, lookback_window=T,
                                   epochs=2, batch_size=32)
    model.fit(X, X)
    assert model._pack.device.type == "cuda"
    assert isinstance(model._pack, Conv1DPack)
    out = model.predict(X)
    assert out.shape == (80 - T + 1, NF) and np.isfinite(out).all()
    serializer.dump(model, str(tmp_path))
    again = serializer.load(str(tmp_path)).predict(X)
    np.testing.assert_array_equal(again, out)
