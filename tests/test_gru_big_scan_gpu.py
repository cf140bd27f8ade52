"""The two-step GRU scan kernels (csrc/gru_seq.hip, ``*_big_kernel``)
against the fp64 oracle ``ops.reference.gru_seq_*_ref``, fed through an
identity: x = mx, Wx = I_3H, b[0] = 0, so mx is a bf16-exact input.
Generator, seeds, weight scale and the bound (``_check``) are those of
tests/test_gru_scan_gpu.py; the backward runs on the oracle's forward.
H: 16 is one unit tile (three waves idle), 80 five tiles dealt unevenly
with a zero K tail both ways, 128 the even case, 256 the halved backward
tile. (B, T): no recurrence; a partial second workgroup; an odd T.
The oracle's fp32 emulation errs on these inputs by hs 1.953e-3, gacts
3.906e-3, dGx 3.906e-3, dGh 4.883e-4, and the kernels on the MI355X
measured the same four figures (docs/kernels.md, "Two-step GRU scan").
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops
from gordo_amd.ops import reference as ref
from test_gru_scan_gpu import _bf, _check, _dev, _inputs, _rand

G = 2


@functools.lru_cache(maxsize=None)
def _big_inputs(B, T, H, sat=False):
    mx = _bf(_rand(G, B, T, 3 * H, seed=15))
    if sat:  # the x side alone holds z and r at +60 (row 0) / -60 (row 1)
        mx[:, 0, :, :2 * H] = 60.0
        mx[:, 1, :, :2 * H] = -60.0
    b = torch.zeros(G, 2, 3 * H, dtype=torch.float64)
    b[:, 1] = _bf(_rand(G, 3 * H, seed=17) * 0.1)
    return dict(mx=mx, b=b,
                Wh=_bf(_rand(G, H, 3 * H, seed=11) * 1.2 / H ** 0.5),
                d_full=_bf(_rand(G, B, T, H, seed=12)),
                d_last=_bf(_rand(G, B, H, seed=13)))


@functools.lru_cache(maxsize=None)
def _oracle(B, T, H, sat=False):
    """(hs, gacts) and, per last_only, (dGx, dGh) on those."""
    i = _big_inputs(B, T, H, sat)
    eye = torch.eye(3 * H, dtype=torch.float64).repeat(G, 1, 1)
    hs, gacts = ref.gru_seq_fwd_ref(i["mx"], eye, i["Wh"], i["b"])
    return (hs, gacts), {lo: ref.gru_seq_bwd_ref(
        i["d_last"] if lo else i["d_full"], gacts, hs, i["Wh"], lo)
        for lo in (False, True)}


def _fwd(i, store_aux=True):
    return ops.gru_seq_fwd_big(_dev(i["mx"]), _dev(i["Wh"]),
                               i["b"][:, 1].to("cuda", torch.float32),
                               store_aux)


@pytest.mark.parametrize("rows", [16, 32, 64])
@pytest.mark.parametrize("B,T", [(1, 1), (33, 2), (20, 5)])
@pytest.mark.parametrize("H", [16, 80, 128, 256])
def test_scans_against_the_oracle(monkeypatch, H, B, T, rows):
    monkeypatch.setenv("GORDO_LSTM_ROWS", str(rows))
    i, (want_fwd, want_bwd) = _big_inputs(B, T, H), _oracle(B, T, H)
    hs, gacts = _fwd(i)
    launch = ops.last_gru_launch()
    assert (launch["family"], launch["rows"], launch["has_dx"], launch[
        "blocks"]) == ("gru_fwd_big", rows, None, G * -(-B // rows))
    _check("hs", hs, want_fwd[0])
    _check("gacts", gacts, want_fwd[1])
    assert torch.equal(_fwd(i, store_aux=False)[0], hs)
    assert torch.equal(_fwd(i)[1], gacts)  # run twice: bitwise equal
    # 64 rows of dGh at H = 256 exceed 160 KB of LDS
    tile = 32 if (rows, H) == (64, 256) else rows
    for last_only in (False, True):
        args = (_dev(i["d_last"] if last_only else i["d_full"]),
                _dev(want_fwd[1]), _dev(want_fwd[0]), _dev(i["Wh"]), last_only)
        dGx, dGh = ops.gru_seq_bwd_big(*args)
        launch = ops.last_gru_launch()
        assert (launch["family"], launch["rows"], launch["has_dx"],
                launch["last_only"]) == ("gru_bwd_big", tile, False, last_only)
        _check("dGx", dGx, want_bwd[last_only][0])
        _check("dGh", dGh, want_bwd[last_only][1])
        again = ops.gru_seq_bwd_big(*args)
        assert torch.equal(again[0], dGx) and torch.equal(again[1], dGh)


@pytest.mark.parametrize("H,F", [(128, 24), (64, 136)])
def test_public_entries_are_the_gemms_plus_the_scans(H, F):
    B, T = 33, 5
    i = _inputs(G, B, T, H, F)
    x, Wx, Wh = _dev(i["x"]), _dev(i["Wx"]), _dev(i["Wh"])
    b = i["b"].to("cuda", torch.float32)
    hs, gacts = ops.gru_seq_fwd(x, Wx, Wh, b)
    assert ops.last_gru_launch()["family"] == "gru_fwd_big"
    mx = ops.grouped_linear_fwd(x.view(G, B * T, F), Wx, b[:, 0], "linear")
    hs2, gacts2 = ops.gru_seq_fwd_big(mx.view(G, B, T, 3 * H), Wh, b[:, 1])
    assert torch.equal(hs, hs2) and torch.equal(gacts, gacts2)
    d = _dev(i["d_full"])
    dGx, dGh, dX = ops.gru_seq_bwd(d, gacts, hs, Wh, False, Wx=Wx)
    assert ops.last_gru_launch()["family"] == "gru_bwd_big"
    dGx2, dGh2 = ops.gru_seq_bwd_big(d, gacts, hs, Wh, False)
    assert torch.equal(dGx, dGx2) and torch.equal(dGh, dGh2)
    want_dX = ops.grouped_linear_bwd_data(dGx.view(G, B * T, 3 * H), Wx)
    assert torch.equal(dX, want_dX.view(G, B, T, F))


def test_saturated_gates_stay_finite_and_exact():
    B, T, H = 4, 4, 16
    i = _big_inputs(B, T, H, sat=True)
    hs, gacts = _fwd(i)
    want_z = _oracle(B, T, H, sat=True)[0][1][..., :H]
    z = gacts[..., :H].double().cpu()
    assert bool((want_z[:, 0] == 1).all()) and bool((want_z[:, 1] < 1e-20).all())
    exact = (want_z == 0) | (want_z == 1)
    assert torch.equal(z[exact], want_z[exact])
    for t in (hs, gacts, *ops.gru_seq_bwd_big(
            _dev(i["d_full"]), gacts, hs, _dev(i["Wh"]), False)):
        assert bool(torch.isfinite(t).all())
