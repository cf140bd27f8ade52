"""Weight regularizers through the packs on the GPU: device packs
against the CPU packs (which test_weight_regularizers.py pins to torch
autograd), pad entries, early stopping with compaction, and the
untouched path of unregularized packs.

Device-vs-CPU tolerances are those of test_gpu_e2e.py (bf16 compute
against the fp32 CPU pack): loss ``rel=0.08, abs=2e-3`` and mean
prediction difference below 0.03 for dense, ``rel=0.1, abs=3e-3`` and
0.05 for LSTM."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import regularizer_cases as rc
from compaction_cases import fit_arm
from gordo_amd import ops
from gordo_amd.engine.pack import DensePack, LSTMPack
from gordo_amd.engine.spec import LayerSpec, ModelSpec
from test_pack_compaction_gpu import _data as compaction_data

MASKED_REG = {"family": "masked", "reg": True}


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def _assert_pads_are_zero(pack):
    """Every entry of a physical tensor outside its logical block."""
    padded = 0
    for name, view in pack.store.views.items():
        logical = pack.store.logical[name]
        if tuple(view.shape) == tuple(logical):
            continue
        assert name not in pack._extractors  # plain dim slicing below
        inside = torch.zeros(view.shape, dtype=torch.bool, device="cuda")
        inside[tuple(slice(0, n) for n in logical)] = True
        assert bool((view[~inside] == 0).all()), name
        assert bool((view[inside] != 0).any()), name
        padded += 1
    return padded


def test_dense_pack_on_device_matches_the_cpu_pack():
    require_hip()
    spec, X = rc.dense_spec(), rc.dense_data()
    seeds = [1, 2, 3]
    cpu = DensePack(spec, rc.DENSE_G, device="cpu", seeds=seeds)
    hist_cpu = cpu.fit(X, X.clone(), **rc.DENSE_FIT)
    plain = DensePack(rc.dense_spec(False), rc.DENSE_G, device="cpu",
                      seeds=seeds)
    hist_plain = plain.fit(X, X.clone(), **rc.DENSE_FIT)
    gpu = DensePack(spec, rc.DENSE_G, device="cuda", seeds=seeds)
    assert gpu.pad8 and gpu.store.reg_table is not None
    hist_gpu = gpu.fit(X.cuda(), X.cuda(), **rc.DENSE_FIT)
    assert ops.last_optimizer_launch() == MASKED_REG
    for e in range(rc.DENSE_EPOCHS):
        for g in range(rc.DENSE_G):
            print("epoch", e, "model", g, "gpu", hist_gpu["loss"][e][g],
                  "cpu", hist_cpu["loss"][e][g], "plain",
                  hist_plain["loss"][e][g])
            assert hist_gpu["loss"][e][g] == pytest.approx(
                hist_cpu["loss"][e][g], rel=0.08, abs=2e-3)
            # the penalty is in it: the plain model's loss is far below
            assert hist_gpu["loss"][e][g] > hist_plain["loss"][e][g] + 0.1
    out_cpu = cpu.predict(X).float().numpy()
    out_gpu = gpu.predict(X.cuda()).float().cpu().numpy()
    assert np.abs(out_cpu - out_gpu).mean() < 0.03
    # the regularized kernel on device follows the CPU pack's, not the
    # plain model's (6 steps of lr * l1 = 0.01 apart)
    w_gpu = np.stack([s["W1"] for s in gpu.states_for_all_models()])
    w_cpu = np.stack([s["W1"] for s in cpu.states_for_all_models()])
    w_plain = np.stack([s["W1"] for s in plain.states_for_all_models()])
    assert np.abs(w_gpu - w_cpu).mean() < 0.25 * np.abs(w_gpu - w_plain).mean()
    # pad8 padded every tensor, and every pad entry is still exactly 0
    assert _assert_pads_are_zero(gpu) == len(gpu.store.views)


def test_lstm_pack_on_device_matches_the_cpu_pack():
    require_hip()
    G, F, H, T, N = 2, 8, 8, 4, 27
    spec = rc.lstm_spec(F, H, T, kernel=(0.01, 0.0), recurrent=(0.0, 0.01))
    X = rc.lstm_data(G, N, F)
    fit = dict(epochs=2, batch_size=8, shuffle=False)
    cpu = LSTMPack(spec, G, device="cpu", seeds=[3, 4])
    assert cpu.n_windows(N) == 24
    hist_cpu = cpu.fit(X, X.clone(), **fit)
    plain = LSTMPack(rc.lstm_spec(F, H, T), G, device="cpu", seeds=[3, 4])
    hist_plain = plain.fit(X, X.clone(), **fit)
    gpu = LSTMPack(spec, G, device="cuda", seeds=[3, 4])
    hist_gpu = gpu.fit(X.cuda(), X.cuda(), **fit)
    assert ops.last_optimizer_launch() == MASKED_REG
    for e in range(2):
        for g in range(G):
            print("epoch", e, "model", g, "gpu", hist_gpu["loss"][e][g],
                  "cpu", hist_cpu["loss"][e][g], "plain",
                  hist_plain["loss"][e][g])
            assert hist_gpu["loss"][e][g] == pytest.approx(
                hist_cpu["loss"][e][g], rel=0.1, abs=3e-3)
            # sum|Wx| alone is about 256 * 0.18, times 0.01
            assert hist_gpu["loss"][e][g] > hist_plain["loss"][e][g] + 0.3
    out_cpu = cpu.predict(X).float().numpy()
    out_gpu = gpu.predict(X.cuda()).float().cpu().numpy()
    assert out_gpu.shape == out_cpu.shape
    assert np.abs(out_cpu - out_gpu).mean() < 0.05


def _compaction_spec():
    """The dense shape of test_pack_compaction_gpu.py (8 -> 8 -> 4 -> 8
    -> 8), with a kernel and a bias regularizer."""
    layers = [
        LayerSpec("dense", 8, "tanh"),
        LayerSpec("dense", 4, "tanh", kernel_l1=1e-4, kernel_l2=1e-3),
        LayerSpec("dense", 8, "tanh", bias_l2=1e-3),
        LayerSpec("dense", 8, "linear"),
    ]
    return ModelSpec(model_type="feedforward", n_features=8,
                     n_features_out=8, layers=layers)


def test_regularized_early_stopping_is_bit_equal_under_compaction():
    require_hip()
    G, seeds = 5, [1, 4, 5, 2, 3]
    spec, X = _compaction_spec(), compaction_data()
    fit = dict(epochs=12, batch_size=128, shuffle=False,
               validation_split=0.2,
               early_stopping={"monitor": "loss", "patience": 1,
                               "min_delta": 0.01})
    snapshot = DensePack(spec, G, device="cuda", seeds=seeds).store.p32.clone()

    def make():
        return DensePack(spec, G, device="cuda", seeds=seeds,
                         init_p32=snapshot)

    off, off_hist = fit_arm(make, X, fit, None)
    assert ops.last_wgrad_launch()["chunks"] == 1  # no atomics: repeatable
    on, on_hist = fit_arm(make, X, fit, 0.5)
    assert ops.last_optimizer_launch() == MASKED_REG
    print("epochs_run", off_hist.epochs_run, "compactions",
          on_hist.compactions)
    assert off_hist.compactions == [] and on_hist.compactions
    assert on_hist.epochs_run == off_hist.epochs_run
    assert on_hist.best_epoch == off_hist.best_epoch
    assert set(on_hist) == set(off_hist) and "val_loss" in on_hist
    for key in off_hist:
        for g in range(G):
            for e in range(off_hist.epochs_run[g]):
                assert on_hist[key][e][g] == off_hist[key][e][g], (key, e, g)
    buffers = lambda p: [p.store.p32, p.store.plp] + [
        t for _k, t in p.store.slots()]
    for a, b in zip(buffers(on), buffers(off)):
        view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(a.view(view), b.view(view))
    assert int(on.store.step_buf) == int(off.store.step_buf)


def test_unregularized_packs_launch_what_they_launched(monkeypatch):
    require_hip()
    calls = []
    real = ops.weight_penalty
    monkeypatch.setattr(
        ops, "weight_penalty",
        lambda *a, **k: calls.append(1) or real(*a, **k))
    X = rc.dense_data().cuda()
    fit = dict(validation_split=0.25, **rc.DENSE_FIT)
    for optimizer, family in (("Adam", "adam"), ("SGD", "opt")):
        spec = rc.dense_spec(False)
        spec.optimizer = optimizer
        pack = DensePack(spec, rc.DENSE_G, device="cuda")
        assert pack.store.reg_table is None
        pack.fit(X, X.clone(), **fit)
        assert ops.last_optimizer_launch() == {"family": family,
                                               "reg": False}
    pack.fit(X, X.clone(), early_stopping={"monitor": "loss", "patience": 5},
             **fit)
    assert ops.last_optimizer_launch() == {"family": "masked", "reg": False}
    assert calls == []
    # and a regularized pack does ask: per batch and per validation pass
    pack = DensePack(rc.dense_spec(), rc.DENSE_G, device="cuda")
    pack.fit(X, X.clone(), **fit)
    assert len(calls) == 3 * rc.DENSE_EPOCHS
    assert ops.last_optimizer_launch() == MASKED_REG
