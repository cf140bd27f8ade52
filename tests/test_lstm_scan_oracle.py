"""The fp64 LSTM scan oracle (gordo_amd.ops.reference.lstm_seq_*_ref)
checked against torch.autograd, on the CPU. The GPU scan tests trust
this oracle, so it is validated here by something that shares no code
with it: differentiating the unrounded forward."""
import pytest
import torch

from gordo_amd.ops import reference as ref


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1)


@pytest.mark.parametrize("last_only", [False, True])
@pytest.mark.parametrize("G,B,T,H,F", [(2, 5, 7, 6, 3), (1, 3, 1, 4, 2)])
def test_bwd_ref_equals_autograd(G, B, T, H, F, last_only):
    """round_points=False in fp64: dG (summed into dWh) and dX equal
    autograd through lstm_seq_fwd_fused_ref to ~1e-10."""
    x = _rand(G, B, T, F, seed=1).requires_grad_()
    Wx = _rand(G, F, 4 * H, seed=2)
    Wh = (_rand(G, H, 4 * H, seed=3) * 0.5).requires_grad_()
    b = (_rand(G, 4 * H, seed=4) * 0.3).requires_grad_()
    dSeq = _rand(G, B, H, seed=5) if last_only else _rand(G, B, T, H, seed=5)

    hs, cs, ga = ref.lstm_seq_fwd_fused_ref(x, Wx, Wh, b,
                                            round_points=False)
    assert hs.dtype == torch.float64
    up = hs[:, :, -1] if last_only else hs
    dx_ag, dWh_ag, db_ag = torch.autograd.grad((up * dSeq).sum(), [x, Wh, b])

    dG, dX = ref.lstm_seq_bwd_ref(dSeq, ga.detach(), cs.detach(),
                                  Wh.detach(), last_only, Wx=Wx,
                                  round_points=False)
    h_prev = torch.cat([torch.zeros_like(hs[:, :, :1]), hs[:, :, :-1]],
                       dim=2).detach()
    dWh = torch.einsum("gbth,gbtn->ghn", h_prev, dG)
    tol = dict(rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(dX, dx_ag, **tol)
    torch.testing.assert_close(dWh, dWh_ag, **tol)
    torch.testing.assert_close(dG.sum(dim=(1, 2)), db_ag, **tol)
    # the Wx-less form returns the same dG alone
    only = ref.lstm_seq_bwd_ref(dSeq, ga.detach(), cs.detach(), Wh.detach(),
                                last_only, round_points=False)
    assert torch.equal(only, dG)


def test_fwd_ref_equals_fused_ref_on_explicit_xw():
    """The two forward forms are the same recurrence: the fused one on
    (x, Wx, b) equals the plain one on xW = x @ Wx + b."""
    G, B, T, H, F = 2, 4, 6, 5, 3
    x, Wx = _rand(G, B, T, F, seed=6), _rand(G, F, 4 * H, seed=7)
    Wh, b = _rand(G, H, 4 * H, seed=8) * 0.5, _rand(G, 4 * H, seed=9)
    xW = torch.einsum("gbtf,gfn->gbtn", x, Wx) + b[:, None, None]
    for a, c in zip(ref.lstm_seq_fwd_ref(xW, Wh, round_points=False),
                    ref.lstm_seq_fwd_fused_ref(x, Wx, Wh, b,
                                               round_points=False)):
        torch.testing.assert_close(a, c, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("round_points", [False, True])
def test_last_only_equals_full_with_zeros(round_points):
    """last_only is the full form with zero upstream grads except at
    T-1 — exactly, rounded or not."""
    G, B, T, H, F = 2, 5, 6, 8, 4
    xW = _rand(G, B, T, 4 * H, seed=10)
    Wh, Wx = _rand(G, H, 4 * H, seed=11) * 0.5, _rand(G, F, 4 * H, seed=12)
    _, cs, ga = ref.lstm_seq_fwd_ref(xW, Wh, round_points=round_points)
    d_last = _rand(G, B, H, seed=13)
    d_full = torch.zeros(G, B, T, H, dtype=torch.float64)
    d_full[:, :, -1] = d_last
    a = ref.lstm_seq_bwd_ref(d_last, ga, cs, Wh, True, Wx=Wx,
                             round_points=round_points)
    b = ref.lstm_seq_bwd_ref(d_full, ga, cs, Wh, False, Wx=Wx,
                             round_points=round_points)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_round_points_land_on_bf16():
    """With round_points=True hs, gacts, dG and dX are bf16-exact; cs
    is not rounded."""
    G, B, T, H, F = 1, 3, 4, 8, 8
    xW = _rand(G, B, T, 4 * H, seed=14)
    Wh, Wx = _rand(G, H, 4 * H, seed=15) * 0.5, _rand(G, F, 4 * H, seed=16)
    hs, cs, ga = ref.lstm_seq_fwd_ref(xW, Wh)
    dG, dX = ref.lstm_seq_bwd_ref(_rand(G, B, T, H, seed=17), ga, cs, Wh,
                                  False, Wx=Wx)
    for t in (hs, ga, dG, dX):
        assert torch.equal(t, t.to(torch.bfloat16).to(torch.float64))
    assert not torch.equal(cs, cs.to(torch.bfloat16).to(torch.float64))
