"""The LSTM scan and pointwise kernels that take a cell activation
(``ACT``: relu, sigmoid, linear beside tanh), by dispatch arm, against
the fp64 oracle of gordo_amd.ops.reference with the same ``act``.

Conventions of tests/test_lstm_scan_arms_gpu.py: every row runs one
kernel through the entry production uses, asserts the launch record
(``ops.last_scan_launch()``: family ``fwd_v4`` / ``bwd_pipe``, the row
tile after LDS halving, ``has_dx`` / ``last_only``) and
``ops.last_scan_activation()``, and compares every output with the
oracle: hs, cs, gacts forward, dG and dX backward. The backward rows
are fed the forward kernel's own gacts / cs.

Inputs are bf16-exact fp64 as that file's ``_inputs``, with Wh scaled
by 1.2/sqrt(H) and Wx by 1.2/sqrt(F): on the CPU this keeps
max|c| <= 2 for all four activations at every shape here (T = 144
included), so the relative term cannot hide an error behind a large
``c`` (at the 0.3 scale of that file linear reaches |c| ~ 20).

Tolerances
----------
The rule of test_lstm_scan_arms_gpu.py, ``err <= max(ATOL[act][output],
2**-6 |want|)``, with ATOL = 4x the largest error of the oracle's own
fp32 emulation (``dtype=torch.float32``) against the fp64 oracle over
the rows below, recomputed on the CPU per activation
(``python tests/test_lstm_scan_act_gpu.py`` prints them):

    act       hs        cs        gacts     dG        dX
    relu      9.766e-4  1.150e-4  3.906e-3  1.953e-3  1.953e-3
    sigmoid   1.953e-3  1.595e-4  3.906e-3  9.766e-4  9.766e-4
    linear    1.953e-3  2.891e-4  3.906e-3  1.953e-3  1.953e-3

(max|c| on the CPU: relu 1.724, sigmoid 1.271, linear 1.725.)

Kernel errors observed on the MI355X (max over the arm's rows):

    arm           act       hs        cs        gacts     dG        dX
    fwd_v4        relu      9.766e-4  1.150e-4  3.906e-3
    fwd_v4        sigmoid   1.953e-3  9.192e-5  3.906e-3
    fwd_v4        linear    1.953e-3  2.891e-4  3.906e-3
    bwd_pipe+dX   relu                                    3.906e-3  1.953e-3
    bwd_pipe+dX   sigmoid                                 9.766e-4  9.766e-4
    bwd_pipe+dX   linear                                  3.906e-3  3.906e-3
    bwd_pipe      relu                                    3.906e-3
    bwd_pipe      sigmoid                                 9.766e-4
    bwd_pipe      linear                                  3.906e-3

Every output holds the bound in every row, with no constant raised.
hs, gacts, dG and dX are single bf16 flips. cs sits on the emulation's
own error because the non-tanh forward instantiations hand the gate
pre-activations to the gate phase in fp32 (docs/kernels.md, "Cell
activation"): with the bf16 tile of the tanh kernel, relu and linear
measured cs 3.588e-3 / 3.651e-3 and missed this bound in 19 rows, since
c = f c + i * bf16(z_g) takes the rounding of z_g undamped.

The pointwise kernels keep the bound rule of
tests/test_gemm_kernels_gpu.py (gemm_cases.check_bf16 / check_f32 with
the 2^-20 floor of the single-``__expf`` functions).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_cases as gc
from gordo_amd import ops
from gordo_amd.ops import reference as ref
from test_lstm_scan_arms_gpu import (
    RTOL, ROW_TILES, HF_FUSED, SAT_ROWS, _bf, _dev, _pipe_rows, _rand,
    _set_env, _v4_rows, require_hip,
)

ACTS = ("relu", "sigmoid", "linear")
# 4x the CPU emulation errors of the docstring
ATOL = {
    "relu": dict(hs=4 * 9.766e-4, cs=4 * 1.150e-4, gacts=4 * 3.906e-3,
                 dG=4 * 1.953e-3, dX=4 * 1.953e-3),
    "sigmoid": dict(hs=4 * 1.953e-3, cs=4 * 1.595e-4, gacts=4 * 3.906e-3,
                    dG=4 * 9.766e-4, dX=4 * 9.766e-4),
    "linear": dict(hs=4 * 1.953e-3, cs=4 * 2.891e-4, gacts=4 * 3.906e-3,
                   dG=4 * 1.953e-3, dX=4 * 1.953e-3),
}
G = 2
BT = [(1, 1), (33, 20), (100, 2)]
LONG = (1, 20, 144, 48, 56)
# where the tanh dispatch of lstm_seq_bwd takes v2 (G * ceil(B/64) >= 256)
V2_SHAPE = (256, 17, 5, 16, 8)
DET_SHAPE = (2, 33, 20, 48, 56)
SAT_SHAPE = (1, 20, 4, 48, 56)


@functools.lru_cache(maxsize=None)
def _inputs(G, B, T, H, F, sat=False):
    """(x, Wx, Wh, b) and the upstream grads of one shape, bf16-exact
    fp64, shared read-only by every row that uses it."""
    Wh = _bf(_rand(G, H, 4 * H, seed=11) * (1.2 / H ** 0.5))
    d_full = _bf(_rand(G, B, T, H, seed=12))
    d_last = _bf(_rand(G, B, H, seed=13))
    x = _bf(_rand(G, B, T, F, seed=15))
    Wx = _bf(_rand(G, F, 4 * H, seed=16) * (1.2 / F ** 0.5))
    b = _bf(_rand(G, 4 * H, seed=17) * 0.1)
    if sat:
        # feature 0 carries the pinned value into every gate
        Wx[:, 0] = 1.0
        x[..., 0] = 0.0
        for r, v in SAT_ROWS.items():
            x[:, r, :, 0] = v
    return dict(x=x, Wx=Wx, Wh=Wh, b=b, d_full=d_full, d_last=d_last)


@functools.lru_cache(maxsize=None)
def _fwd_oracle(shape, act, sat=False, dtype=torch.float64):
    i = _inputs(*shape, sat)
    return ref.lstm_seq_fwd_fused_ref(i["x"], i["Wx"], i["Wh"], i["b"],
                                      dtype=dtype, act=act)


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """A kernel fault surfaces at the next synchronisation: end the run
    there, so no later row launches on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


# observed maxima per (arm, act, output), printed at the end of the run
_SEEN = {}


def _check(arm, act, name, got, want):
    got = got.to(torch.float64).cpu()
    assert got.shape == want.shape
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    err = (got - want).abs()
    atol = ATOL[act][name]
    bound = torch.clamp(RTOL * want.abs(), min=atol)
    key = (arm, act, name)
    _SEEN[key] = max(_SEEN.get(key, 0.0), err.max().item())
    print(f"{arm} {act} {name}: max abs err {err.max().item():.3e} "
          f"(scale {want.abs().max().item():.3e}, atol {atol:.1e})")
    bad = err > bound
    assert not bool(bad.any()), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond "
        f"max({atol:.1e}, 2^-6 |want|); max err {err.max().item():.3e}"
    )


def _expect(family, rows, act, has_dx=None, last_only=None):
    assert ops.last_scan_launch() == dict(
        family=family, rows=rows, hf=None, has_dx=has_dx, last_only=last_only
    )
    assert ops.last_scan_activation() == act


def _fwd(shape, act, sat=False, **kw):
    i = _inputs(*shape, sat)
    return ops.lstm_seq_fwd_fused(_dev(i["x"]), _dev(i["Wx"]), _dev(i["Wh"]),
                                  i["b"].float().cuda(), act=act, **kw)


@functools.lru_cache(maxsize=None)
def _device_forward(shape, act):
    """The forward kernel's own (gacts, cs) for the backward rows."""
    _, cs, ga = _fwd(shape, act)
    return ga, cs


@functools.lru_cache(maxsize=None)
def _bwd_oracle(shape, act, last_only, with_wx):
    i = _inputs(*shape)
    ga, cs = _device_forward(shape, act)
    dSeq = i["d_last"] if last_only else i["d_full"]
    return ref.lstm_seq_bwd_ref(dSeq, ga.cpu(), cs.cpu(), i["Wh"], last_only,
                                Wx=i["Wx"] if with_wx else None, act=act)


def _bwd_args(shape, act, last_only):
    i = _inputs(*shape)
    ga, cs = _device_forward(shape, act)
    return (_dev(i["d_last"] if last_only else i["d_full"]), ga, cs,
            _dev(i["Wh"]))


ROWS = [
    pytest.param((G, B, T, H, F), r, id=f"B{B}T{T}H{H}F{F}-rows{r}")
    for r in ROW_TILES for H, F in HF_FUSED for B, T in BT
] + [pytest.param(LONG, None, id="long-T144")]


def _tile(r):
    return 16 if r is None else r    # pick_rows(1, 20) = 16 unforced


def _env(r):
    return {} if r is None else {"GORDO_LSTM_ROWS": str(r)}


# ---------------------------------------------------------------------------
# the arms
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape,r", ROWS)
def test_fwd_fused(shape, r, act, monkeypatch):
    require_hip()
    want = _fwd_oracle(shape, act)
    _set_env(monkeypatch, _env(r))
    H, F = shape[3], shape[4]
    out = _fwd(shape, act)
    _expect("fwd_v4", _v4_rows(H, F, _tile(r)), act)
    for name, got, w in zip(("hs", "cs", "gacts"), out, want):
        _check("fwd_v4", act, name, got, w)
    lean = _fwd(shape, act, store_aux=False)
    _expect("fwd_v4", _v4_rows(H, F, _tile(r)), act)
    assert len(lean) == 1
    assert torch.equal(lean[0].view(torch.int16), out[0].view(torch.int16))


@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape,r", ROWS)
def test_bwd_fused(shape, r, act, last_only, monkeypatch):
    require_hip()
    want_dG, want_dX = _bwd_oracle(shape, act, last_only, True)
    args = _bwd_args(shape, act, last_only)
    Wx = _dev(_inputs(*shape)["Wx"])
    _set_env(monkeypatch, _env(r))
    dG, dX = ops.lstm_seq_bwd_fused(*args, Wx, last_only, act=act)
    _expect("bwd_pipe", _pipe_rows(shape[3], shape[4], _tile(r), True), act,
            has_dx=True, last_only=last_only)
    _check("bwd_pipe+dX", act, "dG", dG, want_dG)
    _check("bwd_pipe+dX", act, "dX", dX, want_dX)


@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize(
    "shape,r", ROWS + [pytest.param(V2_SHAPE, None, id="v2-shape")])
def test_bwd_bottom(shape, r, act, last_only, monkeypatch):
    """The bottom-layer arm through both entries; ``lstm_seq_bwd``
    skips its v2 / v1 / big routing for a non-tanh ``act``."""
    require_hip()
    want = _bwd_oracle(shape, act, last_only, False)
    args = _bwd_args(shape, act, last_only)
    _set_env(monkeypatch, _env(r))
    # pick_rows(256, 17) = 16, and H = 16 fits any tile
    rows = 16 if shape == V2_SHAPE else _pipe_rows(shape[3], 0, _tile(r),
                                                   False)
    for fn in (ops.lstm_seq_bwd_v3, ops.lstm_seq_bwd):
        dG = fn(*args, last_only, act=act)
        _expect("bwd_pipe", rows, act, has_dx=False, last_only=last_only)
        _check("bwd_pipe", act, "dG", dG, want)
    if shape == V2_SHAPE:
        # the tanh request at this shape does take v2
        ops.lstm_seq_bwd(*args, last_only)
        assert ops.last_scan_launch()["family"] == "bwd_v2"
        assert ops.last_scan_activation() == "tanh"


GUARD = 64  # elements on each side


def _guarded(n_elem):
    """A 16-byte-aligned bf16 view of n_elem elements between two guard
    regions filled with a sentinel."""
    buf = torch.full((n_elem + 2 * GUARD,), -7.0, dtype=torch.bfloat16,
                     device="cuda")
    return buf, buf[GUARD:GUARD + n_elem]


def _guards_intact(buf, n_elem):
    return bool((buf[:GUARD] == -7.0).all()) and bool(
        (buf[GUARD + n_elem:] == -7.0).all())


@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("act", ACTS)
def test_bwd_out_between_guards(act, last_only):
    require_hip()
    shape = (2, 33, 20, 48, 56)
    Gs, B, T, H, F = shape
    args = _bwd_args(shape, act, last_only)
    Wx = _dev(_inputs(*shape)["Wx"])
    want_dG, want_dX = _bwd_oracle(shape, act, last_only, True)
    gbuf, dG = _guarded(Gs * B * T * 4 * H)
    xbuf, dX = _guarded(Gs * B * T * F)
    dG, dX = dG.view(Gs, B, T, 4 * H), dX.view(Gs, B, T, F)
    ops.lstm_seq_bwd_fused_out(*args, Wx, last_only, dG, dX, act=act)
    _expect("bwd_pipe", 16, act, has_dx=True, last_only=last_only)
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, dG.numel()) and _guards_intact(xbuf, dX.numel())
    _check("bwd_pipe+dX", act, "dG", dG, want_dG)
    _check("bwd_pipe+dX", act, "dX", dX, want_dX)

    gbuf, dG = _guarded(Gs * B * T * 4 * H)
    dG = dG.view(Gs, B, T, 4 * H)
    ops.lstm_seq_bwd_v3_out(*args, last_only, dG, act=act)
    _expect("bwd_pipe", 16, act, has_dx=False, last_only=last_only)
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, dG.numel())
    _check("bwd_pipe", act, "dG", dG,
           _bwd_oracle(shape, act, last_only, False))


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def test_explicit_tanh_is_the_default():
    """``act="tanh"`` is bit-equal to the argument omitted, per entry."""
    require_hip()
    shape = (2, 33, 20, 48, 56)
    i = _inputs(*shape)
    fa = (_dev(i["x"]), _dev(i["Wx"]), _dev(i["Wh"]), i["b"].float().cuda())
    base = ops.lstm_seq_fwd_fused(*fa)
    assert ops.last_scan_activation() == "tanh"
    for a, b in zip(base, ops.lstm_seq_fwd_fused(*fa, act="tanh")):
        assert torch.equal(_bits(a), _bits(b))
    _, cs, ga = base
    Wh, Wx = _dev(i["Wh"]), _dev(i["Wx"])
    for last_only in (True, False):
        d = _dev(i["d_last"] if last_only else i["d_full"])
        a = ops.lstm_seq_bwd_fused(d, ga, cs, Wh, Wx, last_only)
        b = ops.lstm_seq_bwd_fused(d, ga, cs, Wh, Wx, last_only, act="tanh")
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
        o1, o2 = torch.empty_like(a[0]), torch.empty_like(a[1])
        ops.lstm_seq_bwd_fused_out(d, ga, cs, Wh, Wx, last_only, o1, o2,
                                   act="tanh")
        assert torch.equal(_bits(o1), _bits(a[0]))
        assert torch.equal(_bits(o2), _bits(a[1]))
        for fn in (ops.lstm_seq_bwd_v3, ops.lstm_seq_bwd):
            p = fn(d, ga, cs, Wh, last_only)
            assert ops.last_scan_activation() == "tanh"
            assert torch.equal(_bits(p),
                               _bits(fn(d, ga, cs, Wh, last_only, act="tanh")))
        o = torch.empty_like(p)
        ops.lstm_seq_bwd_v3_out(d, ga, cs, Wh, last_only, o, act="tanh")
        assert torch.equal(_bits(o), _bits(p))
    g2 = _dev(_rand(2, 33, 4 * 25, seed=30))
    c2 = _rand(2, 33, 25, seed=31).float().cuda()
    f1, f2 = ops.lstm_pointwise_fwd(g2, c2), ops.lstm_pointwise_fwd(
        g2, c2, act="tanh")
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(f1, f2))
    dh = _dev(_rand(2, 33, 25, seed=32))
    b1 = ops.lstm_pointwise_bwd(dh, c2, f1[2], f1[1], c2)
    b2 = ops.lstm_pointwise_bwd(dh, c2, f1[2], f1[1], c2, act="tanh")
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(b1, b2))


@pytest.mark.parametrize("act", ACTS)
def test_unservable_requests_raise(act, monkeypatch):
    """A non-tanh request outside the parametrised kernels raises and
    launches nothing (the launch record stays as it was)."""
    require_hip()
    _set_env(monkeypatch, {})
    # a known record to compare against
    _fwd((2, 1, 1, 8, 8), "tanh")
    before = (ops.last_scan_launch(), ops.last_scan_activation())

    def same():
        return (ops.last_scan_launch(), ops.last_scan_activation()) == before

    def bwd_inputs(B, T, H, F):
        z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
        return (z(2, B, T, H), z(2, B, T, 4 * H),
                torch.zeros(2, B, T, H, device="cuda"), z(2, H, 4 * H),
                z(2, F, 4 * H))

    d, ga, cs, Wh, Wx = bwd_inputs(3, 2, 25, 8)           # H = 25
    for call in (
        lambda: ops.lstm_seq_bwd_fused(d, ga, cs, Wh, Wx, False, act=act),
        lambda: ops.lstm_seq_bwd_v3(d, ga, cs, Wh, False, act=act),
        lambda: ops.lstm_seq_bwd(d, ga, cs, Wh, False, act=act),
    ):
        with pytest.raises(RuntimeError):
            call()
        assert same()
    d, ga, cs, Wh, Wx = bwd_inputs(3, 2, 8, 136)          # F = 136
    with pytest.raises(RuntimeError):
        ops.lstm_seq_bwd_fused(d, ga, cs, Wh, Wx, False, act=act)
    assert same()
    d, ga, cs, Wh, Wx = bwd_inputs(3, 2, 8, 8)            # PIPE off
    monkeypatch.setenv("GORDO_LSTM_PIPE", "0")
    for call in (
        lambda: ops.lstm_seq_bwd_fused(d, ga, cs, Wh, Wx, False, act=act),
        lambda: ops.lstm_seq_bwd_v3(d, ga, cs, Wh, False, act=act),
        lambda: ops.lstm_seq_bwd(d, ga, cs, Wh, False, act=act),
    ):
        with pytest.raises(RuntimeError):
            call()
        assert same()
    assert not ops.lstm_act_scan_available(8, 8)
    monkeypatch.delenv("GORDO_LSTM_PIPE")
    assert ops.lstm_act_scan_available(8, 8)
    assert not ops.lstm_act_scan_available(72, 8)
    assert not ops.lstm_act_scan_available(25, 8)
    assert not ops.lstm_act_scan_available(8, 136)
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):                     # H = 72
        ops.lstm_seq_fwd_fused(z(2, 3, 2, 8), z(2, 8, 288), z(2, 72, 288),
                               torch.zeros(2, 288, device="cuda"), act=act)
    assert same()
    d, ga, cs, Wh, Wx = bwd_inputs(3, 2, 72, 8)
    with pytest.raises(RuntimeError):
        ops.lstm_seq_bwd(d, ga, cs, Wh, False, act=act)
    assert same()


@pytest.mark.parametrize("act", ["relu", "linear"])
def test_fwd_saturation(act, monkeypatch):
    """Rows 0-3 hold the x-side value of every gate at +-60 / +-100
    (SAT_ROWS), at the shape of the tanh saturation rows. With an
    unbounded activation a held +60 makes c grow by about 60 a step and
    |h| reach 900 by the last one. Every output is finite and on the
    oracle; on the held rows a sigmoid gate is exactly 0 or 1 wherever
    the bf16-rounded oracle is, and g, which no exponential touches,
    equals the oracle's bit for bit at every step."""
    require_hip()
    _set_env(monkeypatch, {})
    hs, cs, ga = _fwd(SAT_SHAPE, act, sat=True)
    _expect("fwd_v4", 16, act)
    want = _fwd_oracle(SAT_SHAPE, act, sat=True)
    rows = sorted(SAT_ROWS)
    for name, got, w in zip(("hs", "cs", "gacts"), (hs, cs, ga), want):
        _check("fwd_v4 sat", act, name, got, w)
    H = SAT_SHAPE[3]
    got = ga.cpu()[:, rows].to(torch.float64)
    wga = want[2][:, rows]
    sig = torch.ones(4 * H, dtype=torch.bool)
    sig[2 * H:3 * H] = False
    at01 = ((wga == 0.0) | (wga == 1.0)) & sig
    print(f"sat {act}: {int(at01.sum())} sigmoid gates at 0/1, "
          f"{int((got[at01] != wga[at01]).sum())} differ; g differs at "
          f"{int((got[..., ~sig] != wga[..., ~sig]).sum())} of "
          f"{got[..., ~sig].numel()}")
    assert int(at01.sum()) > 0
    assert torch.equal(got[at01], wga[at01])
    assert torch.equal(got[..., ~sig], wga[..., ~sig])
    for k, r in enumerate(rows):
        g0 = got[:, k, 0, 2 * H:3 * H]
        if SAT_ROWS[r] < 0 and act == "relu":
            assert bool((g0 == 0.0).all())
        else:
            assert bool((g0.abs() > 50.0).all())   # passed through, unsquashed


@pytest.mark.parametrize("r", ROW_TILES)
@pytest.mark.parametrize("act", ACTS)
def test_bitwise_determinism(act, r, monkeypatch):
    require_hip()
    _set_env(monkeypatch, _env(r))
    i = _inputs(*DET_SHAPE)
    first = _fwd(DET_SHAPE, act)
    again = _fwd(DET_SHAPE, act)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, again))
    _, cs, ga = first
    Wh, Wx = _dev(i["Wh"]), _dev(i["Wx"])
    for last_only in (True, False):
        d = _dev(i["d_last"] if last_only else i["d_full"])
        a = ops.lstm_seq_bwd_fused(d, ga, cs, Wh, Wx, last_only, act=act)
        b = ops.lstm_seq_bwd_fused(d, ga, cs, Wh, Wx, last_only, act=act)
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
        p = ops.lstm_seq_bwd_v3(d, ga, cs, Wh, last_only, act=act)
        q = ops.lstm_seq_bwd_v3(d, ga, cs, Wh, last_only, act=act)
        assert torch.equal(_bits(p), _bits(q))


# ---------------------------------------------------------------------------
# the pointwise kernels
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [(1, 1, 8), (2, 33, 25), (3, 70, 64)],
                         ids=lambda s: "G%dB%dH%d" % s)
@pytest.mark.parametrize("act", ACTS)
def test_pointwise(act, shape):
    require_hip()
    Gp, B, H = shape
    gates = gc.rand(Gp, B, 4 * H, seed=35, scale=4.0)
    c_prev = gc.rand_f32(Gp, B, H, seed=36)
    (h, c, ga), (h32, c32, ga32) = ref.lstm_pointwise_fwd_ref(
        gates, c_prev, act)
    got_h, got_c, got_ga = ops.lstm_pointwise_fwd(
        gates.to("cuda", torch.bfloat16), c_prev.cuda(), act=act)
    gc.check_bf16(f"pw_fwd {act} h", got_h, h, h32, gc.EXP_FLOOR)
    gc.check_f32(f"pw_fwd {act} c", got_c, c, c32, gc.EXP_FLOOR)
    gc.check_bf16(f"pw_fwd {act} gact", got_ga, ga, ga32, gc.EXP_FLOOR)
    # backward on its own, from the oracle's forward values
    gact, cf = gc.bf16r(ga.float()), c.float()
    dh = gc.rand(Gp, B, H, seed=37)
    dc_next = gc.rand_f32(Gp, B, H, seed=38, scale=0.1)
    (want_dg, want_dcp), (emu_dg, emu_dcp) = ref.lstm_pointwise_bwd_ref(
        dh, dc_next, gact, cf, c_prev, act)
    got_dg, got_dcp = ops.lstm_pointwise_bwd(
        dh.to("cuda", torch.bfloat16), dc_next.cuda(),
        gact.to("cuda", torch.bfloat16), cf.cuda(), c_prev.cuda(), act=act)
    gc.check_bf16(f"pw_bwd {act} dgates", got_dg, want_dg, emu_dg,
                  gc.EXP_FLOOR)
    gc.check_f32(f"pw_bwd {act} dc_prev", got_dcp, want_dcp, emu_dcp,
                 gc.EXP_FLOOR)


def test_zz_report_observed():
    """Not a check: prints the maxima the rows above observed."""
    for (arm, act, name), v in sorted(_SEEN.items()):
        print(f"observed {arm:12s} {act:8s} {name:6s} {v:.3e}")


# ---------------------------------------------------------------------------
# where ATOL comes from (CPU only; not a test)
# ---------------------------------------------------------------------------


def _emulation_errors(act):
    """Max error of the fp32 emulation against the fp64 oracle, per
    output, over the inputs of every arm row; also max|c|. The backward
    takes the fp64 forward oracle's gacts and cs (as fp32)."""
    worst = dict.fromkeys(("hs", "cs", "gacts", "dG", "dX"), 0.0)
    cmax = 0.0
    # the saturation row is left out: its linear / relu rows hold |h|
    # in the hundreds, where one bf16 flip is 1.0
    for shape in sorted({p.values[0] for p in ROWS} | {DET_SHAPE, V2_SHAPE}):
        hi = _fwd_oracle(shape, act)
        lo = _fwd_oracle(shape, act, dtype=torch.float32)
        for name, a, b in zip(("hs", "cs", "gacts"), hi, lo):
            worst[name] = max(worst[name], (a - b).abs().max().item())
        cmax = max(cmax, hi[1].abs().max().item())
        i = _inputs(*shape)
        ga, cs = hi[2], hi[1].float()
        for last_only in (True, False):
            dSeq = i["d_last"] if last_only else i["d_full"]
            outs = [ref.lstm_seq_bwd_ref(dSeq, ga, cs, i["Wh"], last_only,
                                         Wx=i["Wx"], dtype=dt, act=act)
                    for dt in (torch.float64, torch.float32)]
            for name, a, b in zip(("dG", "dX"), *outs):
                worst[name] = max(worst[name], (a - b).abs().max().item())
    return worst, cmax


if __name__ == "__main__":
    for act in ("tanh",) + ACTS:
        worst, cmax = _emulation_errors(act)
        print(act, " ".join(f"{k} {v:.3e}" for k, v in worst.items()),
              f"| max|c| {cmax:.3f}")
