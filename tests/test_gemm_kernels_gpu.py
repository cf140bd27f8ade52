"""grouped_gemm_kernel (forward, dgrad, accumulate), the wgrad entries
and the pointwise training kernels of gordo_kernels.hip against fp64
oracles, one test row per arm (tests/gemm_cases.py; the arm table is in
docs/kernels.md, "Grouped GEMM arms").

Inputs are rounded to bf16 on the CPU first, so the oracle and the
kernel see the same numbers. The bounds are derived (gemm_cases.py):
``2^-8 |want| + atol`` for a bf16 output and ``max(atol, 2^-22 |want|)``
for an fp32 one, ``atol`` = 4x the fp32 emulation's error (floored at
2^-20 where the kernel evaluates a single-``__expf`` tanh or sigmoid).
The lattice tests use small-integer inputs, for which every product,
partial sum and rounded result is exact, and allow no error at all.
"""
import functools

import pytest
import torch

import gemm_cases as gc
from gordo_amd import ops
from gordo_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def dev(t):
    return t.to("cuda", torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16)


def poison(numel, dtype=torch.bfloat16):
    """Best effort at making "never written" visible: fill a block of
    the output's size with NaN and free it, so the caching allocator
    hands that block to the op's ``torch::empty`` next. Nothing
    guarantees the reuse; when it happens, an element the kernel skips
    reads back NaN and fails the comparison."""
    t = torch.full((numel,), float("nan"), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    del t


def offset_view(t):
    """The same values one element into a larger buffer: contiguous,
    bf16, and not 16-byte aligned."""
    flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def act_floor(act):
    return gc.EXP_FLOOR if act in ("tanh", "sigmoid") else 0.0


# ---------------------------------------------------------------------------
# grouped_linear_fwd
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_inputs(shape):
    G, M, K, N = shape
    return (gc.rand(G, M, K, seed=1), gc.rand(G, K, N, seed=2),
            gc.rand_f32(G, N, seed=3))


@functools.lru_cache(maxsize=None)
def _fwd_oracle(shape, act):
    return ref.grouped_linear_fwd_ref(*_fwd_inputs(shape), act)


@pytest.mark.parametrize("shape,act", gc.FWD_ACT_CASES)
def test_fwd_vs_fp64(shape, act):
    """Every arm row against the fp64 oracle, the output block
    NaN-poisoned first (best effort, see ``poison``): an output tile
    that a wrong block decode leaves unwritten fails here."""
    require_hip()
    X, W, b = _fwd_inputs(shape)
    want, emu = _fwd_oracle(shape, act)
    G, M, K, N = shape
    dX, dW, db = dev(X), dev(W), b.cuda()
    poison(G * M * N)
    got = ops.grouped_linear_fwd(dX, dW, db, act)
    gc.check_bf16(f"fwd {shape} {act}", got, want, emu, act_floor(act))


@pytest.mark.parametrize("act", ["linear", "relu"])
@pytest.mark.parametrize("shape", gc.FWD_SHAPES)
def test_fwd_lattice_exact(shape, act):
    """Ternary operands, integer bias in [-8, 8], K <= 128: |z| <= 136,
    so every product, every fp32 partial sum in any order and the bf16
    result are exact. Any difference is an indexing defect."""
    require_hip()
    G, M, K, N = shape
    X, W = gc.ternary(G, M, K, seed=11), gc.ternary(G, K, N, seed=12)
    b = gc.integers(-8, 8, G, N, seed=13)
    want, emu = ref.grouped_linear_fwd_ref(X, W, b, act)
    assert torch.equal(emu.double(), want)
    poison(G * M * N)
    got = ops.grouped_linear_fwd(dev(X), dev(W), b.cuda(), act)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.cpu(), want.to(torch.bfloat16))


@pytest.mark.parametrize("m_edge", ["first", "last"])
@pytest.mark.parametrize("shape", gc.PROP_SHAPES)
def test_fwd_nan_stays_in_its_row(shape, m_edge):
    """One NaN in A[g0, m0, K-1] (the K tail) makes exactly output row
    (g0, m0) NaN; every other element keeps the clean run's bits."""
    require_hip()
    G, M, K, N = shape
    X, W, b = _fwd_inputs(shape)
    dW, db = dev(W), b.cuda()
    clean = ops.grouped_linear_fwd(dev(X), dW, db, "linear")
    g0, m0 = G - 1, (0 if m_edge == "first" else M - 1)
    Xn = X.clone()
    Xn[g0, m0, K - 1] = float("nan")
    got = ops.grouped_linear_fwd(dev(Xn), dW, db, "linear")
    nan = torch.isnan(got)
    expect = torch.zeros_like(nan)
    expect[g0, m0, :] = True
    assert torch.equal(nan, expect)
    assert not torch.isnan(clean).any()
    assert torch.equal(bits(got)[~expect], bits(clean)[~expect])


# ---------------------------------------------------------------------------
# grouped_linear_bwd_data (B staged from [N][K] rows: both staging forms)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("G,M,inner,Kout", gc.BWD_CASES)
def test_bwd_data_vs_fp64(G, M, inner, Kout):
    require_hip()
    dZ = gc.rand(G, M, inner, seed=4)
    W = gc.rand(G, Kout, inner, seed=5)
    want, emu = ref.grouped_linear_bwd_data_ref(dZ, W)
    d_dZ, d_W = dev(dZ), dev(W)
    poison(G * M * Kout)
    got = ops.grouped_linear_bwd_data(d_dZ, d_W)
    gc.check_bf16(f"bwd_data {(G, M, inner, Kout)}", got, want, emu)


@pytest.mark.parametrize("G,M,inner,Kout", gc.BWD_CASES)
def test_bwd_data_lattice_exact(G, M, inner, Kout):
    require_hip()
    dZ = gc.ternary(G, M, inner, seed=14)
    W = gc.ternary(G, Kout, inner, seed=15)
    want, emu = ref.grouped_linear_bwd_data_ref(dZ, W)
    assert torch.equal(emu.double(), want)
    d_dZ, d_W = dev(dZ), dev(W)
    poison(G * M * Kout)
    got = ops.grouped_linear_bwd_data(d_dZ, d_W)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.cpu(), want.to(torch.bfloat16))


# ---------------------------------------------------------------------------
# grouped_gemm_acc
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("G,M,K,N", gc.ACC_CASES)
def test_gemm_acc_vs_fp64(G, M, K, N):
    require_hip()
    A, B = gc.rand(G, M, K, seed=8), gc.rand(G, K, N, seed=9)
    C0 = gc.rand(G, M, N, seed=10, scale=2.0)
    assert bool((C0 != 0).any())
    want, emu = ref.grouped_gemm_acc_ref(A, B, C0)
    C = dev(C0).contiguous()
    out = ops.grouped_gemm_acc(dev(A), dev(B), C)
    assert out.data_ptr() == C.data_ptr()
    gc.check_bf16(f"gemm_acc {(G, M, K, N)}", C, want, emu)


@pytest.mark.parametrize("G,M,K,N", gc.ACC_CASES)
def test_gemm_acc_lattice_exact(G, M, K, N):
    """Ternary A and B, integer C0 in [-64, 64], K <= 72: |C| <= 136."""
    require_hip()
    A, B = gc.ternary(G, M, K, seed=16), gc.ternary(G, K, N, seed=17)
    C0 = gc.integers(-64, 64, G, M, N, seed=18)
    want, emu = ref.grouped_gemm_acc_ref(A, B, C0)
    assert torch.equal(emu.double(), want)
    C = dev(C0).contiguous()
    ops.grouped_gemm_acc(dev(A), dev(B), C)
    assert torch.equal(C.cpu(), want.to(torch.bfloat16))


# ---------------------------------------------------------------------------
# wgrad entries: ternary inputs make the fp32 sums exact in any atomic
# order, so dW and db are exact on the single-chunk and split-M arms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("G,M,K,N", gc.WGRAD_CASES)
def test_wgrad_lattice_exact(G, M, K, N):
    require_hip()
    X, dZ = gc.ternary(G, M, K, seed=21), gc.ternary(G, M, N, seed=22)
    (want_W, atol_W), (want_b, atol_b) = gc.wgrad_oracle(X, dZ)
    assert atol_W == 0.0 and atol_b == 0.0
    poison(G * K * N, torch.float32)
    got_W, got_b = ops.grouped_linear_wgrad(dev(X), dev(dZ))
    assert got_W.dtype == got_b.dtype == torch.float32
    assert torch.equal(got_W.double().cpu(), want_W)
    assert torch.equal(got_b.double().cpu(), want_b)


@pytest.mark.parametrize("G,B,T,F,H", gc.WGRAD_XH_CASES)
def test_wgrad_xh_and_hprev_lattice_exact(G, B, T, F, H):
    require_hip()
    seq = gc.ternary(G, B * T, F, seed=23)
    hs = gc.ternary(G, B, T, H, seed=24)
    dG = gc.ternary(G, B * T, 4 * H, seed=25)
    h_prev = torch.cat(
        [torch.zeros_like(hs[:, :, :1]), hs[:, :, :-1]], dim=2
    ).reshape(G, B * T, H)
    (want_Wx, _), (want_b, _) = gc.wgrad_oracle(seq, dG)
    (want_Wh, _), _ = gc.wgrad_oracle(h_prev, dG)
    d_seq, d_hs, d_dG = dev(seq), dev(hs), dev(dG)
    got_Wx, got_Wh, got_b = ops.grouped_wgrad_xh(d_seq, d_hs, d_dG, T)
    assert torch.equal(got_Wx.double().cpu(), want_Wx)
    assert torch.equal(got_Wh.double().cpu(), want_Wh)
    assert torch.equal(got_b.double().cpu(), want_b)
    sep_Wh, sep_b = ops.grouped_linear_wgrad_hprev(d_hs, d_dG, T)
    assert torch.equal(sep_Wh.double().cpu(), want_Wh)
    assert torch.equal(sep_b.double().cpu(), want_b)


# ---------------------------------------------------------------------------
# Offset views: a contiguous bf16 view whose storage offset is odd
# passes through the launchers unchanged. The host must then choose the
# element-wise staging; both forms load the same values, so the output
# is bit-equal to the aligned call.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("shape", gc.PROP_SHAPES)
def test_fwd_offset_view_bit_equal(shape, which):
    require_hip()
    X, W, b = _fwd_inputs(shape)
    dX, dW, db = dev(X), dev(W), b.cuda()
    base = ops.grouped_linear_fwd(dX, dW, db, "tanh")
    if which == "A":
        dX = offset_view(dX)
    else:
        dW = offset_view(dW)
    got = ops.grouped_linear_fwd(dX, dW, db, "tanh")
    assert torch.equal(bits(got), bits(base))


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("shape", gc.PROP_SHAPES)
def test_bwd_data_offset_view_bit_equal(shape, which):
    """(G, M, K, N) read as dZ [G, M, K], W [G, N, K]: K is the inner
    dimension, so K = 40 has both 16-byte stagings to lose."""
    require_hip()
    G, M, K, N = shape
    dZ, W = dev(gc.rand(G, M, K, seed=4)), dev(gc.rand(G, N, K, seed=5))
    base = ops.grouped_linear_bwd_data(dZ, W)
    if which == "A":
        dZ = offset_view(dZ)
    else:
        W = offset_view(W)
    got = ops.grouped_linear_bwd_data(dZ, W)
    assert torch.equal(bits(got), bits(base))


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("shape", gc.PROP_SHAPES)
def test_gemm_acc_offset_view_bit_equal(shape, which):
    require_hip()
    G, M, K, N = shape
    A, B = dev(gc.rand(G, M, K, seed=8)), dev(gc.rand(G, K, N, seed=9))
    C0 = dev(gc.rand(G, M, N, seed=10, scale=2.0))
    base = ops.grouped_gemm_acc(A, B, C0.clone())
    if which == "A":
        A = offset_view(A)
    else:
        B = offset_view(B)
    got = ops.grouped_gemm_acc(A, B, C0.clone())
    assert torch.equal(bits(got), bits(base))


def test_window_gather_offset_view_bit_equal():
    """F = 8 with X one element into its buffer: the 16-byte copy is
    not legal, the element loop must serve it."""
    require_hip()
    G, N, F, B, T = 2, 60, 8, 5, 7
    X = dev(gc.rand(G, N, F, seed=70))
    idx = torch.tensor([[0, N - T, 3, 17, 29]] * G, dtype=torch.int32,
                       device="cuda")
    base = ops.window_gather(X, idx, T)
    got = ops.window_gather(offset_view(X), idx, T)
    rows = idx.long().unsqueeze(-1) + torch.arange(T, device="cuda")
    want = X.gather(
        1, rows.reshape(G, B * T, 1).expand(G, B * T, F)
    ).view(G, B, T, F)
    assert torch.equal(bits(base), bits(want))
    assert torch.equal(bits(got), bits(want))


# ---------------------------------------------------------------------------
# Pointwise kernels: one element count past the launch cap, so the
# grid-stride loop takes its second trip; edges; saturation
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _act_l1_inputs():
    n = gc.CAP_POINTWISE + 3
    dA, Y = gc.rand(n, seed=31), gc.rand(n, seed=32)
    # +0, -0 and tiny magnitudes either side of 0 (2^-100: every
    # product with them is still a normal number), at the front and in
    # the three second-trip elements
    Y[:4] = torch.tensor([0.0, -0.0, 2.0 ** -100, -(2.0 ** -100)])
    Y[n - 3:] = torch.tensor([2.0 ** -100, -0.0, 0.0])
    dA[:4] = torch.tensor([0.75, -0.75, 0.5, 0.5])
    dA[n - 3:] = torch.tensor([0.5, 0.75, -0.75])
    return dA, Y


@pytest.mark.parametrize("l1", [0.0, 1e-4])
@pytest.mark.parametrize("act", gc.ACTS)
def test_act_l1_bwd_second_trip_and_zero_edges(act, l1):
    require_hip()
    dA, Y = _act_l1_inputs()
    n = Y.numel()
    want, emu = ref.act_l1_bwd_ref(dA, Y, act, l1)
    d_dA, d_Y = dev(dA), dev(Y)
    poison(n)
    got = ops.act_l1_bwd(d_dA, d_Y, act, l1)
    gc.check_bf16(f"act_l1_bwd {act} l1={l1}", got, want, emu)
    # sign(+-0) = 0: the l1 term vanishes; act'(0) is 1, 1, 0 (relu), 0
    # (sigmoid from its output), all exactly
    zero = Y == 0
    assert int(zero.sum()) >= 4 and bool(zero[n - 2:].all())
    slope = {"linear": 1.0, "tanh": 1.0, "relu": 0.0, "sigmoid": 0.0}[act]
    assert torch.equal(got.cpu().float()[zero], dA[zero] * slope)
    if act == "relu":
        # relu' is 1 just above 0 and 0 just below
        tiny = gc.bf16r(dA[2] + torch.tensor(l1)).item()
        assert got[2].item() == tiny and got[3].item() == 0.0


@functools.lru_cache(maxsize=None)
def _mse_inputs():
    per_g = gc.CAP_MSE + 5
    return gc.rand(2, per_g, 1, seed=33), gc.rand(2, per_g, 1, seed=34)


@pytest.mark.parametrize("real_n", [-1, 100003])
def test_mse_bwd_second_trip(real_n):
    require_hip()
    Y, T = _mse_inputs()
    (want_loss, want_dY), (emu_loss, emu_dY) = ref.mse_bwd_ref(Y, T, real_n)
    dY_, dT_ = dev(Y), dev(T)
    poison(Y.numel())
    loss, dY = ops.mse_bwd(dY_, dT_, real_n)
    gc.check_f32(f"mse loss real_n={real_n}", loss, want_loss, emu_loss)
    gc.check_bf16(f"mse dY real_n={real_n}", dY, want_dY, emu_dY)


def test_mse_bwd_lattice_exact():
    """Y - T in {-1, 0, 1} with the divisor 2^17: every square is 0 or
    1, every partial sum an integer below 2^24 and the scaling by 2^-17
    exact, so the loss is exact in any reduction order. The fp32 bound
    above has to allow for a long running sum; this one notices a
    single element counted twice or not at all."""
    require_hip()
    per_g = gc.CAP_MSE + 5
    Y = gc.ternary(2, per_g, 1, seed=42)
    T = gc.ternary(2, per_g, 1, seed=43)
    T[Y * T < 0] = 0.0   # keep |Y - T| <= 1
    d = (Y - T).double()
    assert d.abs().max().item() == 1.0 and bool(d[:, -5:].abs().sum() > 0)
    loss, dY = ops.mse_bwd(dev(Y), dev(T), 2 ** 17)
    assert torch.equal(loss.double().cpu(),
                       (d * d).sum(dim=(1, 2)) * 2.0 ** -17)
    assert torch.equal(dY.cpu().double(), d * 2.0 ** -16)


def test_mse_bwd_models_do_not_mix():
    """Model 1's loss and gradient do not see model 0's data: model 0
    is scaled by 128 with a NaN in its last element (the neighbour of
    model 1's first), and model 1 must still meet its own bound."""
    require_hip()
    Y, T = _mse_inputs()
    (want_loss, want_dY), (emu_loss, emu_dY) = ref.mse_bwd_ref(Y, T)
    Y2 = Y.clone()
    Y2[0] *= 128
    Y2[0, -1, 0] = float("nan")
    loss, dY = ops.mse_bwd(dev(Y2), dev(T))
    assert torch.isnan(loss[0]).item()
    gc.check_f32("mse loss[1]", loss[1:], want_loss[1:], emu_loss[1:])
    gc.check_bf16("mse dY[1]", dY[1:], want_dY[1:], emu_dY[1:])
    base_loss, base_dY = ops.mse_bwd(dev(Y), dev(T))
    assert torch.equal(bits(dY[1]), bits(base_dY[1]))


LSTM_ROWS, LSTM_H = 13798, 38   # rows * H = 524324 > 524288


@functools.lru_cache(maxsize=None)
def _lstm_pw_case():
    gates = gc.rand(2, LSTM_ROWS // 2, 4 * LSTM_H, seed=35, scale=4.0)
    c_prev = gc.rand_f32(2, LSTM_ROWS // 2, LSTM_H, seed=36)
    fwd = ref.lstm_pointwise_fwd_ref(gates, c_prev)
    return gates, c_prev, fwd


def test_lstm_pointwise_fwd_second_trip():
    require_hip()
    gates, c_prev, ((h, c, ga), (h32, c32, ga32)) = _lstm_pw_case()
    assert gates.numel() // 4 > gc.CAP_POINTWISE
    d_gates, d_cp = dev(gates), c_prev.cuda()
    poison(h.numel())
    got_h, got_c, got_ga = ops.lstm_pointwise_fwd(d_gates, d_cp)
    gc.check_bf16("lstm_pw_fwd h", got_h, h, h32, gc.EXP_FLOOR)
    gc.check_f32("lstm_pw_fwd c", got_c, c, c32, gc.EXP_FLOOR)
    gc.check_bf16("lstm_pw_fwd gact", got_ga, ga, ga32, gc.EXP_FLOOR)


def test_lstm_pointwise_bwd_second_trip():
    """From the oracle's forward values (gact rounded to bf16, c in
    fp32), so the backward kernel is checked on its own."""
    require_hip()
    gates, c_prev, ((_h, c, ga), _emu) = _lstm_pw_case()
    gact, c32 = gc.bf16r(ga.float()), c.float()
    dh = gc.rand(*c.shape, seed=37)
    dc_next = gc.rand_f32(*c.shape, seed=38, scale=0.1)
    (want_dg, want_dcp), (emu_dg, emu_dcp) = ref.lstm_pointwise_bwd_ref(
        dh, dc_next, gact, c32, c_prev
    )
    args = (dev(dh), dc_next.cuda(), dev(gact), c32.cuda(), c_prev.cuda())
    poison(want_dg.numel())
    got_dg, got_dcp = ops.lstm_pointwise_bwd(*args)
    gc.check_bf16("lstm_pw_bwd dgates", got_dg, want_dg, emu_dg,
                  gc.EXP_FLOOR)
    gc.check_f32("lstm_pw_bwd dc_prev", got_dcp, want_dcp, emu_dcp,
                 gc.EXP_FLOOR)


def test_lstm_pointwise_saturation():
    """Pre-activations from {+-30, +-100}, every combination over the
    four gates, c_prev = +-1. Wherever the oracle's gate rounds to
    exactly 0, 1 or -1 in bf16 the kernel's must equal it: tanh at all
    four values, sigmoid at +30 and +-100. sigmoid(-30) = 9.36e-14 is
    a normal bf16 number, not 0; there the kernel keeps a relative
    bound: 2^-8 for the bf16 rounding plus 2^-16 for ``__expf(30)``,
    whose argument scaling 30 * log2(e) rounds in fp32 (43 * 2^-24 in
    the exponent, about 2^-19 of the value) before the hardware exp2
    adds its own ulp. No NaN anywhere, forward or backward."""
    require_hip()
    vals = torch.tensor([30.0, 100.0, -30.0, -100.0])
    grid = torch.cartesian_prod(vals, vals, vals, vals)       # [256, 4]
    gates = torch.cat([grid, grid]).reshape(1, 512, 4)         # H = 1
    c_prev = torch.cat([torch.ones(256), -torch.ones(256)]).reshape(1, 512, 1)
    (h, c, ga), (h32, c32, ga32) = ref.lstm_pointwise_fwd_ref(gates, c_prev)
    got_h, got_c, got_ga = ops.lstm_pointwise_fwd(dev(gates), c_prev.cuda())
    for name, t in (("h", got_h), ("c", got_c), ("gact", got_ga)):
        assert not torch.isnan(t).any(), name
    want_ga = ga.to(torch.bfloat16)
    exact = (want_ga == 0) | (want_ga.abs() == 1)
    assert int((~exact).sum()) == 3 * 128  # the sigmoid(-30) entries
    ga_cpu = got_ga.cpu()
    assert torch.equal(ga_cpu[exact], want_ga[exact])
    rel = ((ga_cpu[~exact].double() - ga[~exact]) / ga[~exact]).abs()
    print(f"sigmoid(-30) max rel err {rel.max().item():.3e}")
    assert rel.max().item() <= 2.0 ** -8 + 2.0 ** -16
    gc.check_bf16("sat h", got_h, h, h32, gc.EXP_FLOOR)
    gc.check_f32("sat c", got_c, c, c32, gc.EXP_FLOOR)

    dh = gc.rand(1, 512, 1, seed=39)
    dc_next = gc.rand_f32(1, 512, 1, seed=40)
    got_dg, got_dcp = ops.lstm_pointwise_bwd(
        dev(dh), dc_next.cuda(), got_ga, got_c, c_prev.cuda()
    )
    assert not torch.isnan(got_dg).any() and not torch.isnan(got_dcp).any()
    (want_dg, want_dcp), (emu_dg, emu_dcp) = ref.lstm_pointwise_bwd_ref(
        dh, dc_next, ga_cpu.float(), got_c.cpu(), c_prev
    )
    gc.check_bf16("sat dgates", got_dg, want_dg, emu_dg, gc.EXP_FLOOR)
    gc.check_f32("sat dc_prev", got_dcp, want_dcp, emu_dcp, gc.EXP_FLOOR)


def test_adam_step_second_trip_and_device_step():
    """Steps 1, 2, 3 and, with ``step_buf`` set to 999, step 1000, each
    from the kernel's own previous fp32 state against the fp64 oracle.
    The ``step`` argument is deliberately wrong on the last call: the
    bias correction must follow ``step_buf``."""
    require_hip()
    n = gc.CAP_ADAM + 7
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-7
    p = gc.rand_f32(n, seed=41)
    pd, md, vd = p.cuda(), torch.zeros(n, device="cuda"), torch.zeros(
        n, device="cuda")
    plp = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    step_buf = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t, arg_step in ((1, 1), (2, 2), (3, 3), (1000, 4)):
        if t == 1000:
            step_buf.fill_(999)
        g = gc.rand_f32(n, seed=50 + t, scale=1.0 / min(t, 4) ** 2)
        before = (pd.cpu(), md.cpu(), vd.cpu())
        (wp, wm, wv), (ep, em, ev) = ref.adam_step_ref(
            *before[:1], g, *before[1:], lr, b1, b2, eps, t
        )
        ops.adam_step(pd, g.cuda(), md, vd, lr, b1, b2, eps, arg_step, plp,
                      step_buf=step_buf)
        assert int(step_buf) == t
        gc.check_f32(f"adam step {t} m", md, wm, em)
        gc.check_f32(f"adam step {t} v", vd, wv, ev)
        gc.check_f32(f"adam step {t} p", pd, wp, ep)
        # the mirror is the kernel's own p rounded to nearest: within
        # half a bf16 ulp of it
        assert torch.equal(bits(plp), bits(pd.to(torch.bfloat16)))
        if t == 1000:
            # what following the argument would have given is far
            # outside the bound, so the check above discriminates
            (xp, _, _), _ = ref.adam_step_ref(
                *before[:1], g, *before[1:], lr, b1, b2, eps, arg_step
            )
            gap = (xp - wp).abs()
            assert gap.max().item() > 1e-3
