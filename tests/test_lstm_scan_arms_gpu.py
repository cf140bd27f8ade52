"""Every LSTM scan kernel family, by dispatch arm, against the fp64
oracle of gordo_amd.ops.reference (lstm_seq_*_ref).

Each row of the arm tables runs one kernel through the entry point that
production uses to reach it, asserts ``ops.last_scan_launch()`` (family,
row tile, and for v2 its HF) so the row cannot silently drift onto
another kernel, and compares every output with the oracle: hs, cs and
gacts forward, dG (and dX) backward. The oracle is fp64 with bf16
rounding at the rounding points the scans share (h, gacts, dG, dX); the
backward rows feed it the forward kernel's own gacts / cs so forward
error does not leak into the backward figures.

Tolerances
----------
``err <= max(ATOL[output], RTOL * |want|)`` per element.

* ``ATOL`` is 4x the largest error of the oracle's own fp32 emulation
  (``*_ref(dtype=torch.float32)``) against the fp64 oracle over the
  inputs of every arm row below (``_emulation_errors()`` recomputes the
  figures on the CPU).
* ``RTOL = 2**-6`` is the floor of 2 bf16 ulps of the element: a single
  rounding flip is legitimate, and the kernels' fast ``__expf`` adds a
  little.

CPU-measured emulation errors (fp32 vs fp64 oracle, max over all rows):

    hs 1.953e-3   cs 9.933e-4   gacts 3.906e-3   dG 3.906e-3   dX 9.766e-4

(3.906e-3 is one bf16 ulp in [0.5, 1), 1.953e-3 one in [0.25, 0.5): the
emulation differs from the oracle by single rounding flips.)

Kernel errors observed on the MI355X (max over the family's rows):

    family     hs        cs        gacts     dG        dX
    fwd_v1     3.906e-3  2.562e-3  3.906e-3
    fwd_v2     1.953e-3  4.948e-4  3.906e-3
    fwd_v3     3.906e-3  2.562e-3  3.906e-3
    fwd_v4     3.906e-3  2.981e-3  3.906e-3
    fwd_big    3.906e-3  2.869e-3  3.906e-3
    bwd_v1                                   3.906e-3
    bwd_v2                                   1.953e-3
    bwd_v3                                   3.906e-3
    bwd_v5                                   3.906e-3  3.906e-3
    bwd_pipe                                 3.906e-3  3.906e-3
    bwd_big                                  3.906e-3

Every family stays inside the 4x bound with no constant raised. v2
matches the oracle's rounding points exactly (gate pre-activations and
the dh carry stay in fp32 registers); the other families also pass the
pre-activations and the dh carry through bf16 in LDS, which is where
their larger cs figures come from.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops
from gordo_amd.ops import reference as ref
from scan_cases import (  # noqa: F401 (re-exported to the act tests)
    Arm, FWD_ARMS, BWD_ARMS, V4_ARMS, FUSED_BWD_ARMS, SAT_ARMS, HF_FUSED,
    ROW_TILES, _params, _pipe_rows, _set_env, _v4_rows,
)

RTOL = 2.0 ** -6
# 4x the CPU emulation errors of the docstring
ATOL = {
    "hs": 4 * 1.953e-3,
    "cs": 4 * 9.933e-4,
    "gacts": 4 * 3.906e-3,
    "dG": 4 * 3.906e-3,
    "dX": 4 * 9.766e-4,
}


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def _bf(t):
    """Round to bf16, keep fp64: what the kernel sees, exactly."""
    return t.to(torch.bfloat16).to(torch.float64)


def _dev(t):
    return t.to("cuda", torch.bfloat16)


# rows of the saturation cases and the x-side gate value each is held at
SAT_ROWS = {0: 60.0, 1: -60.0, 2: 100.0, 3: -100.0}


@functools.lru_cache(maxsize=None)
def _inputs(G, B, T, H, F=0, sat=False):
    """bf16-exact fp64 inputs of one shape, shared (read-only) by every
    row that uses it. F > 0: (x, Wx, Wh, b) for the fused entry points;
    else (xW, Wh). ``sat`` pins the x-side gate value of SAT_ROWS."""
    wh_scale = 0.3 if H <= 64 else 2.4 / H ** 0.5
    Wh = _bf(_rand(G, H, 4 * H, seed=11) * wh_scale)
    d_full = _bf(_rand(G, B, T, H, seed=12))
    d_last = _bf(_rand(G, B, H, seed=13))
    if F == 0:
        xW = _bf(_rand(G, B, T, 4 * H, seed=14))
        if sat:
            for r, v in SAT_ROWS.items():
                xW[:, r] = v
        return dict(xW=xW, Wh=Wh, d_full=d_full, d_last=d_last)
    x = _bf(_rand(G, B, T, F, seed=15))
    Wx = _bf(_rand(G, F, 4 * H, seed=16) * 0.3)
    b = _bf(_rand(G, 4 * H, seed=17) * 0.1)
    if sat:
        # feature 0 carries the pinned value into every gate: Wx[0] = 1,
        # x[..., 0] = the value on SAT_ROWS and 0 elsewhere
        Wx[:, 0] = 1.0
        x[..., 0] = 0.0
        for r, v in SAT_ROWS.items():
            x[:, r, :, 0] = v
    return dict(x=x, Wx=Wx, Wh=Wh, b=b, d_full=d_full, d_last=d_last)


@functools.lru_cache(maxsize=None)
def _fwd_oracle(G, B, T, H, F=0, sat=False, dtype=torch.float64):
    i = _inputs(G, B, T, H, F, sat)
    if F == 0:
        return ref.lstm_seq_fwd_ref(i["xW"], i["Wh"], dtype=dtype)
    return ref.lstm_seq_fwd_fused_ref(i["x"], i["Wx"], i["Wh"], i["b"],
                                      dtype=dtype)


def _check(name, got, want):
    got = got.to(torch.float64).cpu()
    assert got.shape == want.shape
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    err = (got - want).abs()
    bound = torch.clamp(RTOL * want.abs(), min=ATOL[name])
    print(f"{name}: max abs err {err.max().item():.3e} "
          f"(scale {want.abs().max().item():.3e}, atol {ATOL[name]:.1e})")
    bad = err > bound
    assert not bool(bad.any()), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond "
        f"max({ATOL[name]:.1e}, 2^-6 |want|); max err {err.max().item():.3e}"
    )


def _expect_launch(family, rows, hf=None, has_dx=None, last_only=None):
    assert ops.last_scan_launch() == dict(
        family=family, rows=rows, hf=hf, has_dx=has_dx, last_only=last_only
    )


def _run_fwd(arm, sat=False, store_aux=True):
    G, B, T, H, F = arm.shape
    i = _inputs(G, B, T, H, F, sat)
    if arm.entry == "fused":
        return ops.lstm_seq_fwd_fused(_dev(i["x"]), _dev(i["Wx"]),
                                      _dev(i["Wh"]), i["b"].float().cuda(),
                                      store_aux=store_aux)
    fn = {"public": ops.lstm_seq_fwd, "v2": ops.lstm_seq_fwd_v2,
          "v3": ops.lstm_seq_fwd_v3}[arm.entry]
    return fn(_dev(i["xW"]), _dev(i["Wh"]))


@functools.lru_cache(maxsize=None)
def _device_forward(G, B, T, H, F):
    """One forward per shape for the backward rows (no switches set):
    the kernel's own (gacts, cs), on the device, read-only."""
    i = _inputs(G, B, T, H, F)
    if F:
        _, cs, ga = ops.lstm_seq_fwd_fused(
            _dev(i["x"]), _dev(i["Wx"]), _dev(i["Wh"]), i["b"].float().cuda()
        )
    else:
        _, cs, ga = ops.lstm_seq_fwd(_dev(i["xW"]), _dev(i["Wh"]))
    return ga, cs


@functools.lru_cache(maxsize=None)
def _bwd_oracle(G, B, T, H, F, last_only):
    i = _inputs(G, B, T, H, F)
    ga, cs = _device_forward(G, B, T, H, F)
    dSeq = i["d_last"] if last_only else i["d_full"]
    return ref.lstm_seq_bwd_ref(dSeq, ga.cpu(), cs.cpu(), i["Wh"], last_only,
                                Wx=i["Wx"] if F else None)


def _run_bwd(arm, last_only):
    G, B, T, H, F = arm.shape
    i = _inputs(G, B, T, H, F)
    ga, cs = _device_forward(G, B, T, H, F)
    dSeq = _dev(i["d_last"] if last_only else i["d_full"])
    Wh = _dev(i["Wh"])
    if arm.entry == "fused":
        return ops.lstm_seq_bwd_fused(dSeq, ga, cs, Wh, _dev(i["Wx"]),
                                      last_only)
    fn = {"public": ops.lstm_seq_bwd, "v2": ops.lstm_seq_bwd_v2,
          "v3": ops.lstm_seq_bwd_v3}[arm.entry]
    return fn(dSeq, ga, cs, Wh, last_only)


# ---------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("arm", _params(FWD_ARMS))
def test_fwd_arm(arm, monkeypatch):
    require_hip()
    _set_env(monkeypatch, arm.env)
    hs, cs, ga = _run_fwd(arm)
    _expect_launch(arm.family, arm.rows, arm.hf)
    want = _fwd_oracle(*arm.shape)
    for name, got, w in zip(("hs", "cs", "gacts"), (hs, cs, ga), want):
        _check(name, got, w)


@pytest.mark.parametrize("store_aux", [True, False])
@pytest.mark.parametrize("arm", _params(V4_ARMS))
def test_fwd_v4_arm(arm, store_aux, monkeypatch):
    require_hip()
    _set_env(monkeypatch, arm.env)
    out = _run_fwd(arm, store_aux=store_aux)
    _expect_launch(arm.family, arm.rows)
    want = _fwd_oracle(*arm.shape)
    assert len(out) == (3 if store_aux else 1)
    for name, got, w in zip(("hs", "cs", "gacts"), out, want):
        _check(name, got, w)


@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("arm", _params(BWD_ARMS))
def test_bwd_arm(arm, last_only, monkeypatch):
    require_hip()
    want = _bwd_oracle(*arm.shape, last_only)
    _set_env(monkeypatch, arm.env)
    dG = _run_bwd(arm, last_only)
    if arm.family == "bwd_pipe":
        _expect_launch(arm.family, arm.rows, has_dx=False,
                       last_only=last_only)
    else:
        _expect_launch(arm.family, arm.rows, arm.hf)
    _check("dG", dG, want)


@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("arm", _params(FUSED_BWD_ARMS))
def test_bwd_fused_arm(arm, last_only, monkeypatch):
    require_hip()
    want_dG, want_dX = _bwd_oracle(*arm.shape, last_only)
    _set_env(monkeypatch, arm.env)
    dG, dX = _run_bwd(arm, last_only)
    if arm.family == "bwd_pipe":
        _expect_launch(arm.family, arm.rows, has_dx=True,
                       last_only=last_only)
    else:
        _expect_launch(arm.family, arm.rows)
    _check("dG", dG, want_dG)
    _check("dX", dX, want_dX)


@pytest.mark.parametrize("arm", _params(SAT_ARMS))
def test_fwd_saturation(arm, monkeypatch):
    """Rows whose x-side gate value sits at +-60 / +-100: every output
    stays finite and on the oracle, sigmoid lands on exactly 0 or 1 and
    tanh on exactly +-1 (``1 - 2 / (e + 1)`` with e = inf or 0)."""
    require_hip()
    _set_env(monkeypatch, arm.env)
    hs, cs, ga = _run_fwd(arm, sat=True)
    _expect_launch(arm.family, arm.rows, arm.hf)
    want = _fwd_oracle(*arm.shape, sat=True)
    for name, got, w in zip(("hs", "cs", "gacts"), (hs, cs, ga), want):
        _check(name, got, w)
    H = arm.shape[3]
    ga = ga.float().cpu()
    for r, v in SAT_ROWS.items():
        sig = torch.cat([ga[:, r, :, :2 * H], ga[:, r, :, 3 * H:]], dim=-1)
        tanh = ga[:, r, :, 2 * H:3 * H]
        assert bool((tanh == (1.0 if v > 0 else -1.0)).all())
        if v > 0:
            assert bool((sig == 1.0).all())
        elif v == -100.0:
            # exp(100) overflows fp32: 1 / (1 + inf) is exactly 0;
            # sigmoid(-60) = 8.8e-27 is a normal bf16 and stays nonzero
            assert bool((sig == 0.0).all())


def test_v2_agrees_with_v3_and_pipe():
    """At one shared shape (H = 48) the v2 kernels and the row-tiled
    ones agree with each other within the bound each keeps against the
    oracle."""
    require_hip()
    G, B, T, H = 2, 70, 12, 48
    i = _inputs(G, B, T, H)
    xW, Wh = _dev(i["xW"]), _dev(i["Wh"])
    out2 = ops.lstm_seq_fwd_v2(xW, Wh)
    _expect_launch("fwd_v2", 64, 3)
    out3 = ops.lstm_seq_fwd_v3(xW, Wh)
    _expect_launch("fwd_v3", 16)
    want = _fwd_oracle(G, B, T, H)
    for name, a, b, w in zip(("hs", "cs", "gacts"), out2, out3, want):
        _check(name, a, w)
        _check(name, b, w)
        _check(name, a, b.to(torch.float64).cpu())
    ga, cs = _device_forward(G, B, T, H, 0)
    for last_only in (True, False):
        dSeq = _dev(i["d_last"] if last_only else i["d_full"])
        d2 = ops.lstm_seq_bwd_v2(dSeq, ga, cs, Wh, last_only)
        _expect_launch("bwd_v2", 64, 3)
        dp = ops.lstm_seq_bwd_v3(dSeq, ga, cs, Wh, last_only)
        _expect_launch("bwd_pipe", 16, has_dx=False, last_only=last_only)
        w = _bwd_oracle(G, B, T, H, 0, last_only)
        _check("dG", d2, w)
        _check("dG", dp, w)
        _check("dG", d2, dp.to(torch.float64).cpu())


# ---------------------------------------------------------------------------
# where ATOL comes from (CPU only; not a test)
# ---------------------------------------------------------------------------


def _emulation_errors():
    """Max error of the fp32 emulation against the fp64 oracle, per
    output, over the inputs of every arm row. The backward takes the
    fp64 forward oracle's gacts and cs (as fp32) in the place of the
    kernel's."""
    worst = dict.fromkeys(ATOL, 0.0)
    shapes = {(a.shape, False) for a in
              FWD_ARMS + BWD_ARMS + V4_ARMS + FUSED_BWD_ARMS}
    shapes |= {(a.shape, True) for a in SAT_ARMS}
    for (G, B, T, H, F), sat in sorted(shapes):
        hi = _fwd_oracle(G, B, T, H, F, sat)
        lo = _fwd_oracle(G, B, T, H, F, sat, dtype=torch.float32)
        for name, a, b in zip(("hs", "cs", "gacts"), hi, lo):
            worst[name] = max(worst[name], (a - b).abs().max().item())
        if sat:
            continue
        i = _inputs(G, B, T, H, F)
        ga, cs = hi[2], hi[1].float()
        for last_only in (True, False):
            dSeq = i["d_last"] if last_only else i["d_full"]
            outs = []
            for dtype in (torch.float64, torch.float32):
                o = ref.lstm_seq_bwd_ref(dSeq, ga, cs, i["Wh"], last_only,
                                         Wx=i["Wx"] if F else None,
                                         dtype=dtype)
                outs.append(o if F else (o,))
            for name, a, b in zip(("dG", "dX"), *outs):
                worst[name] = max(worst[name], (a - b).abs().max().item())
    return worst


if __name__ == "__main__":
    for k, v in _emulation_errors().items():
        print(f"{k}: {v:.3e}  (x4 = {4 * v:.3e})")
