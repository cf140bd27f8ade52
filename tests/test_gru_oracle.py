"""The GRU cell on the CPU: the fp64 scan oracle against torch.nn.GRU
plus autograd, the raw-spec parser, and one train_batch of the CPU pack
(reference ops) against a plain fp32 autograd model.

torch.nn.GRU is the same cell (reset applied after h @ Wh, two biases)
with gate order r, z, n; ``_to_torch`` permutes the blocks.
"""
import numpy as np
import pytest
import torch

from gordo_amd.engine.pack import GRUPack
from gordo_amd.machine.model.models import _parse_raw_spec
from gordo_amd.ops import reference as ref


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def _to_torch(w, H):
    """[..., 3H] in z, r, n order -> torch's [3H, ...] in r, z, n."""
    z, r, n = w[..., :H], w[..., H:2 * H], w[..., 2 * H:]
    return torch.cat([r, z, n], dim=-1).T.contiguous()


def _from_torch(w, H):
    r, z, n = w[:H], w[H:2 * H], w[2 * H:]
    return torch.cat([z, r, n], dim=0).T


@pytest.mark.parametrize("B,T,H,F", [(3, 5, 8, 8), (2, 4, 24, 16)])
@pytest.mark.parametrize("last_only", [False, True])
def test_scan_oracle_equals_torch_gru(B, T, H, F, last_only):
    x = _rand(1, B, T, F, seed=1)
    Wx = _rand(1, F, 3 * H, seed=2) * 0.5
    Wh = _rand(1, H, 3 * H, seed=3) * 0.5
    b = _rand(1, 2, 3 * H, seed=4) * 0.3
    dSeq = _rand(1, B, H, seed=5) if last_only else _rand(1, B, T, H, seed=5)

    gru = torch.nn.GRU(F, H, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(_to_torch(Wx[0], H))
        gru.weight_hh_l0.copy_(_to_torch(Wh[0], H))
        gru.bias_ih_l0.copy_(_to_torch(b[0, 0], H))
        gru.bias_hh_l0.copy_(_to_torch(b[0, 1], H))
    xt = x[0].clone().requires_grad_(True)
    out, _ = gru(xt)
    ((out[:, -1] if last_only else out) * dSeq[0]).sum().backward()

    hs, gacts = ref.gru_seq_fwd_ref(x, Wx, Wh, b, round_points=False)
    dGx, dGh, dX = ref.gru_seq_bwd_ref(dSeq, gacts, hs, Wh, last_only, Wx=Wx,
                                       round_points=False)
    h_prev = torch.cat([torch.zeros_like(hs[:, :, :1]), hs[:, :, :-1]], 2)
    tol = dict(rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(hs[0], out.detach(), **tol)
    torch.testing.assert_close(dX[0], xt.grad, **tol)
    torch.testing.assert_close(torch.einsum("btf,btn->fn", x[0], dGx[0]),
                               _from_torch(gru.weight_ih_l0.grad, H), **tol)
    torch.testing.assert_close(torch.einsum("bth,btn->hn", h_prev[0], dGh[0]),
                               _from_torch(gru.weight_hh_l0.grad, H), **tol)
    torch.testing.assert_close(dGx[0].sum((0, 1)),
                               _from_torch(gru.bias_ih_l0.grad, H), **tol)
    torch.testing.assert_close(dGh[0].sum((0, 1)),
                               _from_torch(gru.bias_hh_l0.grad, H), **tol)


def _raw(*layers):
    return {"keras.Sequential": {"layers": [
        {f"keras.layers.{name}": kw} for name, kw in layers]}}


def test_raw_gru_spec_parses():
    spec = _parse_raw_spec(
        _raw(("GRU", dict(units=6, return_sequences=True,
                          recurrent_regularizer={"L2": {"l2": 0.01}})),
             ("GRU", dict(units=5)), ("Dense", dict(units=5))),
        {}, 5, 5, lookback_window=6)
    assert spec.model_type == "gru" and spec.recurrent
    assert [l.kind for l in spec.layers] == ["gru", "gru", "dense"]
    assert [l.return_sequences for l in spec.layers[:2]] == [True, False]
    assert spec.layers[0].recurrent_l2 == 0.01


@pytest.mark.parametrize("layers,match", [
    ([("GRU", dict(units=4, reset_after=False))], "reset_after"),
    ([("GRU", dict(units=4, activation="relu"))], "GRU activation"),
    ([("GRU", dict(units=4, recurrent_activation="hard_sigmoid"))],
     "recurrent_activation"),
    ([("GRU", dict(units=4, recurrent_dropout=0.1))], "recurrent_dropout"),
    ([("GRU", dict(units=4, return_sequences=True)),
      ("LSTM", dict(units=4))], "mixes GRU and LSTM"),
])
def test_raw_gru_spec_rejects(layers, match):
    with pytest.raises(ValueError, match=match):
        _parse_raw_spec(_raw(*layers, ("Dense", dict(units=5))), {}, 5, 5)


def _plain_torch(pack, Xw, Tgt):
    """(loss[G], grads) of an fp32 autograd model on the pack's logical
    weights."""
    st = {n: torch.tensor(np.stack([pack.state_for_model(g)[n]
                                    for g in range(pack.G)]),
                          requires_grad=True) for n in pack.param_names()}
    seq = Xw
    for i, (_f, H, _rs) in enumerate(pack.lstm_meta_logical):
        h = torch.zeros(pack.G, Xw.shape[1], H)
        outs = []
        for t in range(Xw.shape[2]):
            mx = torch.bmm(seq[:, :, t], st[f"Wx{i}"]) + st[f"bl{i}"][:, :1]
            mh = torch.bmm(h, st[f"Wh{i}"]) + st[f"bl{i}"][:, 1:]
            z = torch.sigmoid(mx[..., :H] + mh[..., :H])
            r = torch.sigmoid(mx[..., H:2 * H] + mh[..., H:2 * H])
            n = torch.tanh(mx[..., 2 * H:] + r * mh[..., 2 * H:])
            h = z * h + (1 - z) * n
            outs.append(h)
        seq = torch.stack(outs, 2)
    y = torch.bmm(seq[:, :, -1], st["Wd"]) + st["bd"].unsqueeze(1)
    loss = ((y - Tgt) ** 2).mean(dim=(1, 2))
    loss.sum().backward()
    return loss.detach(), {n: v.grad for n, v in st.items()}


@pytest.mark.parametrize("pad8", ["1", "0"])
def test_cpu_pack_step_matches_plain_torch(monkeypatch, pad8):
    """Logical widths 5 -> 6 -> 5. Loss and gradients within the bound
    of the same comparison in tests/test_lstm_activation.py; after the
    step every pad entry of every parameter is exactly 0 (a CPU pack has
    none, so the physical arrays are the logical ones)."""
    from gordo_amd.engine.spec import LayerSpec, ModelSpec

    monkeypatch.setenv("GORDO_PAD8", pad8)
    spec = ModelSpec(
        model_type="gru", n_features=5, n_features_out=5, lookback_window=4,
        layers=[LayerSpec(kind="gru", units=6),
                LayerSpec(kind="gru", units=5, return_sequences=False),
                LayerSpec(kind="dense", units=5, activation="linear")])
    pack = GRUPack(spec, G=2, device="cpu", seeds=[3, 4])
    g = torch.Generator().manual_seed(7)
    Xw = torch.rand(2, 7, 4, 5, generator=g)
    Tgt = torch.rand(2, 7, 5, generator=g)
    want_loss, want = _plain_torch(pack, Xw, Tgt)
    loss = pack.train_batch(Xw, Tgt)
    np.testing.assert_allclose(loss.numpy(), want_loss.numpy(), rtol=1e-4)
    for name in pack.param_names():
        assert float(want[name].abs().max()) > 0, name
        np.testing.assert_allclose(pack.store.gviews[name].numpy(),
                                   want[name].numpy(), rtol=2e-3, atol=1e-5)
        for m in range(2):
            view = pack.store.views[name][m]
            mask = torch.zeros_like(view)
            pack._insert_logical(name, mask, np.ones(
                pack.store.logical[name][1:], dtype=np.float32))
            assert bool((view[mask == 0] == 0).all()), name
