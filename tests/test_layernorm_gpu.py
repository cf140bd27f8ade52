"""The grouped LayerNormalization kernels (csrc/layernorm.hip) against the
fp64 oracle, by dispatch arm, and a LayerNormalization raw spec through
the engine on the GPU.

Bound ("Bound" in docs/kernels.md): inputs are rounded to bf16 before the
oracle; a bf16 output holds |got - want| <= 2^-8 |want| + atol with atol =
4 x the oracle's own fp32-emulation error on those inputs, an fp32 output
max(atol, 2^-22 |want|). The pack comparison uses the bounds of
tests/test_conv1d_pack_gpu.py.
"""
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops
from gordo_amd.engine.pack import DensePack
from gordo_amd.machine.model.models import (
    KerasRawModelRegressor, _parse_raw_spec)
from gordo_amd.ops import reference as ref
from test_lstm_activation_gpu import (
    GRAD_BOUND, LOSS_BOUND, _deviation, _logical_grads)

RAW = {"keras.Sequential": {"layers": [
    {"keras.layers.Dense": {"units": 6, "activation": "tanh"}},
    {"keras.layers.LayerNormalization": {}},
    {"keras.layers.Dense": {"units": 5}},
]}}

# (G, B, Fp, real_f, data), lanes, vec, chunks (forward and backward alike
# until a backward workgroup walks more than one row group: the last case)
CASES = [
    ((1, 1, 1, 1, "randn"), 4, False, (1, 1)),       # F = 1
    ((2, 3, 7, 7, "randn"), 4, False, (1, 1)),       # element-wise arm
    ((1, 1, 8, 8, "randn"), 4, True, (1, 1)),        # single chunk
    ((3, 5, 56, 50, "randn"), 8, True, (1, 1)),      # non-zero pad columns
    ((2, 17, 64, 64, "randn"), 8, True, (1, 1)),
    ((1, 33, 136, 136, "randn"), 32, True, (5, 5)),  # dead chunks
    ((2, 9, 512, 512, "randn"), 64, True, (3, 3)),   # full
    ((1, 70, 24, 24, "randn"), 4, True, (2, 2)),     # 16 rows per wave, tail
    ((2, 300, 40, 40, "randn"), 8, True, (10, 10)),  # chunks through reduce
    ((64, 70, 264, 260, "nanpad"), 64, True, (18, 6)),  # 3 passes per chunk
    ((2, 40, 64, 64, "cancel"), 8, True, (2, 2)),    # one-pass variance fails
]


@pytest.mark.parametrize("shape,lanes,vec,chunks", CASES)
@pytest.mark.parametrize("center,scale", [(True, True), (False, False)])
def test_kernels_against_the_oracle(shape, lanes, vec, chunks, center, scale):
    assert ops.hip_available()
    G, B, Fp, real_f, data = shape
    g = torch.Generator().manual_seed(G * 1000 + B + Fp)
    if data == "cancel":  # exact in bf16; var ~ 0.17 under a mean of 100
        x = 99.5 + 0.5 * torch.randint(0, 3, (G, B, Fp), generator=g).float()
    else:
        x = torch.randn(G, B, Fp, generator=g) * 2 + 0.5
    x = x.bfloat16()
    dy = torch.randn(G, B, Fp, generator=g).bfloat16()
    gamma = torch.randn(G, Fp, generator=g) if scale else None
    beta = torch.randn(G, Fp, generator=g) if center else None
    if data == "nanpad":  # pad columns of every operand hold NaN
        for t in (x, dy, gamma, beta):
            if t is not None:
                t[..., real_f:] = float("nan")
    dev = lambda t: None if t is None else t.cuda()

    def run(store_stats=True):
        y, mean, rstd = ops.layer_norm_fwd(dev(x), dev(gamma), dev(beta),
                                           real_f, 1e-3, store_stats)
        rec_f = ops.last_layer_norm_launch()
        if not store_stats:
            return y
        dx, dgamma, dbeta = ops.layer_norm_bwd(dev(dy), dev(x), mean, rstd,
                                               dev(gamma), real_f, center)
        return (y, mean, rstd, dx, dgamma, dbeta), rec_f, \
            ops.last_layer_norm_launch()

    got, rec_f, rec_b = run()
    assert rec_f == {"family": "ln_fwd", "lanes": lanes, "vec": vec,
                     "chunks": chunks[0], "blocks": G * chunks[0]}
    assert rec_b == {"family": "ln_bwd", "lanes": lanes, "vec": vec,
                     "chunks": chunks[1], "blocks": G * chunks[1]}
    assert rec_f == ops.layer_norm_plan("fwd", G, B, Fp)
    assert rec_b == ops.layer_norm_plan("bwd", G, B, Fp)
    mean, rstd = got[1].cpu(), got[2].cpu()
    want_f, emu_f = ref.layer_norm_fwd_ref(x, gamma, beta, real_f, 1e-3)
    want_b, emu_b = ref.layer_norm_bwd_ref(dy, x, mean, rstd, gamma, real_f,
                                           center)
    names = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")
    for name, t, want, emu in zip(names, got, want_f + want_b, emu_f + emu_b):
        if want is None:
            assert t is None, name
            continue
        t = t.cpu()
        atol = 4 * float((emu.double() - want).abs().max())
        err = (t.double() - want).abs()
        if t.dtype == torch.bfloat16:
            over = err - 2.0 ** -8 * want.abs()
            bound = torch.full_like(err, atol)
        else:
            over = err
            bound = torch.clamp(2.0 ** -22 * want.abs(), min=atol)
        print(f"{shape} {name}: max error {float(over.max()):.3e}, "
              f"atol {atol:.3e}")
        assert bool((over <= bound).all()), name
        if name in ("y", "dx", "dgamma", "dbeta"):
            assert bool((t[..., real_f:] == 0).all()), name
    # stats off: the same y; a second run: the same bits everywhere
    assert torch.equal(run(store_stats=False), got[0])
    for t, again in zip(got, run()[0]):
        assert t is None or torch.equal(t, again)


def test_misaligned_view_takes_the_element_arm():
    G, B, Fp = 2, 9, 40
    g = torch.Generator().manual_seed(5)
    x = torch.randn(G, B, Fp, generator=g).bfloat16().cuda()
    dy = torch.randn(G, B, Fp, generator=g).bfloat16().cuda()
    gamma = torch.randn(G, Fp, generator=g).cuda()
    beta = torch.randn(G, Fp, generator=g).cuda()

    def off(t):  # the same values, 2 bytes past a 16-byte boundary
        flat = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
        flat[1:1 + t.numel()].copy_(t.reshape(-1))
        return flat[1:1 + t.numel()].view(t.shape)

    y, mean, rstd = ops.layer_norm_fwd(x, gamma, beta, Fp, 1e-3)
    assert ops.last_layer_norm_launch()["vec"]
    y2, mean2, rstd2 = ops.layer_norm_fwd(off(x), gamma, beta, Fp, 1e-3)
    assert not ops.last_layer_norm_launch()["vec"]
    bwd = ops.layer_norm_bwd(dy, x, mean, rstd, gamma, Fp)
    bwd2 = ops.layer_norm_bwd(off(dy), off(x), mean, rstd, gamma, Fp)
    assert not ops.last_layer_norm_launch()["vec"]
    for a, b in zip((y, mean, rstd) + tuple(bwd), (y2, mean2, rstd2) + tuple(bwd2)):
        assert torch.equal(a, b)


def test_wide_layers_are_refused_with_the_planners_message():
    assert ops.layer_norm_plan("fwd", 2, 16, 520) is None
    assert "Fp <= 512" in ops.layer_norm_refusal("bwd", 2, 16, 520)
    spec = _parse_raw_spec({"keras.Sequential": {"layers": [
        {"keras.layers.Dense": {"units": 520}},
        {"keras.layers.LayerNormalization": {}},
        {"keras.layers.Dense": {"units": 5}}]}}, {}, 5, 5)
    with pytest.raises(ValueError, match="Fp <= 512"):
        DensePack(spec, G=1, device="cuda")


def _one_step(device):
    pack = DensePack(_parse_raw_spec(RAW, {}, 5, 5), G=3, device=device,
                     seeds=[1, 2, 3])
    g = torch.Generator().manual_seed(21)
    X = torch.rand(3, 40, 5, generator=g)
    Tb = torch.rand(3, 40, 5, generator=g)
    loss = pack.train_batch(pack._to_compute(X), pack._to_compute(Tb))
    return pack, loss.float().cpu().numpy(), _logical_grads(pack)


def test_gpu_pack_step_matches_cpu_pack(monkeypatch):
    monkeypatch.delenv("GORDO_PAD8", raising=False)
    gpu = _one_step("cuda")
    pack = gpu[0]
    assert pack.pad8 and pack.layer_meta[0][:2] == (8, 8)
    assert ops.last_layer_norm_launch()["family"] == "ln_bwd"
    loss_dev, grad_dev = _deviation(gpu, _one_step("cpu"))
    print(f"layernorm gpu vs cpu: loss deviation {loss_dev:.3e} (bound "
          f"{LOSS_BOUND:.3e}), gradient deviation {grad_dev:.3e} (bound "
          f"{GRAD_BOUND:.3e})")
    assert loss_dev <= LOSS_BOUND and grad_dev <= GRAD_BOUND
    n_pad = 0
    for name in pack.param_names():
        for m in range(3):
            view = pack.store.views[name][m]
            mask = torch.zeros_like(view)
            pack._insert_logical(name, mask, np.ones(
                pack.store.logical[name][1:], dtype=np.float32))
            n_pad += int((mask == 0).sum())
            assert bool((view[mask == 0] == 0).all()), name
            assert bool((pack.store.gviews[name][m][mask == 0] == 0).all())
    assert n_pad > 0


def test_fit_predict_and_pickle_round_trip():
    X = np.random.default_rng(0).random((80, 5)).astype("float32")
    model = KerasRawModelRegressor(kind={"spec": RAW}, epochs=2, batch_size=32)
    model.fit(X, X)
    assert model._pack.device.type == "cuda"
    assert "ln0_gamma" in model._pack.param_names()
    out = model.predict(X)
    assert out.shape == (80, 5) and np.isfinite(out).all()
    again = pickle.loads(pickle.dumps(model)).predict(X)
    np.testing.assert_array_equal(again, out)


def test_stopped_models_layernorm_parameters_stay_put():
    """Model 0 learns tiny targets: its loss stops improving by min_delta
    at once and it ends early. A second fit capped at that epoch ends it
    in the same state, so equal bits say nothing moved it afterwards."""
    g = torch.Generator().manual_seed(3)
    X = torch.rand(3, 96, 5, generator=g) * torch.tensor(
        [0.01, 3.0, 3.0]).view(3, 1, 1)
    es = {"monitor": "loss", "patience": 1, "min_delta": 0.01}

    def fit(epochs):
        pack = DensePack(_parse_raw_spec(RAW, {}, 5, 5), G=3, device="cuda",
                         seeds=[1, 2, 3])
        hist = pack.fit(X.cuda(), X.cuda(), epochs=epochs, batch_size=32,
                        shuffle=False, early_stopping=es)
        return pack, hist

    long_pack, hist = fit(8)
    assert hist.epochs_run[0] < max(hist.epochs_run)
    short_pack, _ = fit(hist.epochs_run[0])
    for name, init in (("ln0_gamma", 1.0), ("ln0_beta", 0.0)):
        stopped = long_pack.store.views[name][0]
        assert bool((stopped[:6] != init).all()), name  # it did train
        assert torch.equal(stopped, short_pack.store.views[name][0]), name
