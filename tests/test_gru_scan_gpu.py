"""The fused GRU scan kernels (csrc/gru_seq.hip) against the fp64 oracle
(``ops.reference.gru_seq_*_ref``), per row tile and backward arm.

The bound is the rule of tests/test_lstm_scan_arms_gpu.py:
``err <= max(ATOL[output], 2^-6 |want|)`` per element, where ATOL is 4x
the largest error of the oracle's own fp32 emulation against the fp64
oracle over the inputs of every shape below (``_atol`` computes it on the
CPU, once). The backward rows run on the oracle's forward outputs, so
forward error does not leak into the backward figures. Weights are scaled
as in that file (Wh by 1.2/sqrt(H), Wx by 1.2/sqrt(F)).

Shapes (G, B, T, H, F), the smallest at which each mechanism can go
wrong: a single row and step; the bench layer with a row tail and zero
blocks straddling a k-step; the largest LDS (row tile halved); F >> H;
the workload's lookback for drift over T.

Figures (max over all shapes and row tiles): the fp32 emulation errs by
hs 1.953e-3, gacts 3.906e-3, dGx 3.906e-3, dGh 1.953e-3, dX 3.906e-3;
the kernels on the MI355X measured exactly the same five figures (single
bf16 rounding flips), inside the 4x bound.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops
from gordo_amd.ops import reference as ref

RTOL = 2.0 ** -6
SHAPES = [(1, 1, 1, 8, 8), (2, 33, 20, 48, 56), (2, 100, 2, 64, 128),
          (3, 17, 5, 8, 128), (2, 20, 144, 48, 56)]
ARMS = [(dx, lo) for dx in (False, True) for lo in (False, True)]


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def _bf(t):
    """Round to bf16, keep fp64: what the kernel sees, exactly."""
    return t.to(torch.bfloat16).to(torch.float64)


def _dev(t):
    return t.to("cuda", torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _inputs(G, B, T, H, F, sat=False):
    i = dict(x=_bf(_rand(G, B, T, F, seed=15)),
             Wx=_bf(_rand(G, F, 3 * H, seed=16) * 1.2 / F ** 0.5),
             Wh=_bf(_rand(G, H, 3 * H, seed=11) * 1.2 / H ** 0.5),
             b=_bf(_rand(G, 2, 3 * H, seed=17) * 0.1),
             d_full=_bf(_rand(G, B, T, H, seed=12)),
             d_last=_bf(_rand(G, B, H, seed=13)))
    if sat:
        # feature 0 alone drives the x side of z and r: +60 on row 0,
        # -60 on row 1, 0 elsewhere
        i["Wx"][:, 0, :2 * H] = 1.0
        i["Wx"][:, 0, 2 * H:] = 0.0
        i["x"][..., 0] = 0.0
        i["x"][:, 0, :, 0] = 60.0
        i["x"][:, 1, :, 0] = -60.0
    return i


@functools.lru_cache(maxsize=None)
def _oracle(shape, dtype=torch.float64, sat=False):
    """fwd (hs, gacts) and, per arm, bwd (dGx, dGh[, dX]) on the fp64
    forward's outputs."""
    i = _inputs(*shape, sat)
    fwd = ref.gru_seq_fwd_ref(i["x"], i["Wx"], i["Wh"], i["b"], dtype=dtype)
    hs, gacts = _oracle(shape, sat=sat)[0] if dtype != torch.float64 else fwd
    bwd = {
        (dx, lo): ref.gru_seq_bwd_ref(
            i["d_last"] if lo else i["d_full"], gacts, hs, i["Wh"], lo,
            Wx=i["Wx"] if dx else None, dtype=dtype)
        for dx, lo in ARMS
    }
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def _atol():
    worst = dict.fromkeys(("hs", "gacts", "dGx", "dGh", "dX"), 0.0)
    for shape in SHAPES:
        (f64, b64), (f32, b32) = _oracle(shape), _oracle(shape, torch.float32)
        pairs = list(zip(("hs", "gacts"), f32, f64))
        for arm in ARMS:
            pairs += zip(("dGx", "dGh", "dX"), b32[arm], b64[arm])
        for name, got, want in pairs:
            worst[name] = max(worst[name],
                              float((got.double() - want).abs().max()))
    print("fp32 emulation errors:", worst)
    return {k: 4 * v for k, v in worst.items()}


def _check(name, got, want):
    got = got.to(torch.float64).cpu()
    assert got.shape == want.shape
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    err = (got - want).abs()
    atol = _atol()[name]
    print(f"{name}: max abs err {err.max().item():.3e} "
          f"(scale {want.abs().max().item():.3e}, atol {atol:.1e})")
    bad = err > torch.clamp(RTOL * want.abs(), min=atol)
    assert not bool(bad.any()), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond "
        f"max({atol:.1e}, 2^-6 |want|); max err {err.max().item():.3e}")


def _fwd(i, store_aux=True):
    return ops.gru_seq_fwd(_dev(i["x"]), _dev(i["Wx"]), _dev(i["Wh"]),
                           i["b"].to("cuda", torch.float32), store_aux)


def _rows(rows, shape, halves):
    """The (64, 128) tile exceeds 160 KB of LDS at 64 rows."""
    return 32 if rows == 64 and shape[3:] == (64, 128) and halves else rows


@pytest.mark.parametrize("rows", [16, 32, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward(monkeypatch, shape, rows):
    assert ops.hip_available()
    monkeypatch.setenv("GORDO_LSTM_ROWS", str(rows))
    i = _inputs(*shape)
    hs, gacts = _fwd(i)
    launch = ops.last_gru_launch()
    assert (launch["family"], launch["rows"]) == (
        "gru_fwd", _rows(rows, shape, True))
    want_hs, want_ga = _oracle(shape)[0]
    _check("hs", hs, want_hs)
    _check("gacts", gacts, want_ga)
    (hs_only,) = _fwd(i, store_aux=False)
    assert torch.equal(hs_only, hs)


@pytest.mark.parametrize("rows", [16, 32, 64])
@pytest.mark.parametrize("has_dx,last_only", ARMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_backward(monkeypatch, shape, has_dx, last_only, rows):
    assert ops.hip_available()
    monkeypatch.setenv("GORDO_LSTM_ROWS", str(rows))
    i = _inputs(*shape)
    (hs, gacts), bwd = _oracle(shape)
    out = ops.gru_seq_bwd(
        _dev(i["d_last"] if last_only else i["d_full"]), _dev(gacts),
        _dev(hs), _dev(i["Wh"]), last_only,
        Wx=_dev(i["Wx"]) if has_dx else None)
    launch = ops.last_gru_launch()
    assert (launch["family"], launch["rows"], launch["has_dx"],
            launch["last_only"]) == (
        "gru_bwd", _rows(rows, shape, has_dx), has_dx, last_only)
    assert len(out) == (3 if has_dx else 2)
    for name, got, want in zip(("dGx", "dGh", "dX"), out,
                               bwd[(has_dx, last_only)]):
        _check(name, got, want)


def test_saturated_gates_stay_finite_and_exact():
    shape = (1, 4, 4, 16, 8)
    i = _inputs(*shape, sat=True)
    hs, gacts = _fwd(i)
    (want_hs, want_ga), bwd = _oracle(shape, sat=True)
    z, want_z = gacts[..., :16].double().cpu(), want_ga[..., :16]
    assert bool((want_z[:, 0] == 1).all()) and bool((want_z[:, 1] < 1e-20).all())
    exact = (want_z == 0) | (want_z == 1)
    assert torch.equal(z[exact], want_z[exact])
    out = ops.gru_seq_bwd(_dev(i["d_full"]), gacts, hs, _dev(i["Wh"]), False,
                          Wx=_dev(i["Wx"]))
    for t in (hs, gacts) + tuple(out):
        assert bool(torch.isfinite(t).all())


def test_run_twice_is_bitwise_equal():
    i = _inputs(2, 33, 20, 48, 56)
    a, b = _fwd(i), _fwd(i)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    args = (_dev(i["d_full"]), a[1], a[0], _dev(i["Wh"]), False)
    c = ops.gru_seq_bwd(*args, Wx=_dev(i["Wx"]))
    d = ops.gru_seq_bwd(*args, Wx=_dev(i["Wx"]))
    assert all(torch.equal(x, y) for x, y in zip(c, d))
