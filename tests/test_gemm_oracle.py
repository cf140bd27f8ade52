"""The fp64 oracles of the grouped GEMM and pointwise training kernels
(gordo_amd.ops.reference: ``*_ref``) validated on the CPU: against
``torch.bmm`` in fp64 and autograd at 1e-12, and the bound helpers of
gemm_cases.py on hand-made cases. The device tests
(test_gemm_kernels_gpu.py) compare the HIP kernels with these oracles.
"""
import pytest
import torch

import gemm_cases as gc
from gordo_amd.ops import reference as ref

TOL = 1e-12


def _close(a, b, tol=TOL):
    assert a.dtype == torch.float64 and a.shape == b.shape
    assert (a - b.double()).abs().max().item() <= tol


def _act64(z, act):
    return ref.apply_act(z, ref.act_code(act))


@pytest.mark.parametrize("act", gc.ACTS)
@pytest.mark.parametrize("G,M,K,N", [(1, 1, 1, 1), (3, 9, 33, 5),
                                     (2, 70, 40, 70)])
def test_fwd_ref_vs_bmm(G, M, K, N, act):
    X, W = gc.rand(G, M, K, seed=1), gc.rand(G, K, N, seed=2)
    b = gc.rand_f32(G, N, seed=3)
    want, emu = ref.grouped_linear_fwd_ref(X, W, b, act)
    z = torch.bmm(X.double(), W.double()) + b.double().unsqueeze(1)
    _close(want, _act64(z, act))
    assert emu.dtype == torch.float32
    assert (emu.double() - want).abs().max().item() < 1e-5


def test_fwd_ref_is_not_transposed():
    """W[k, n] = k + 100 n with one-hot rows of X picks W[k, :]."""
    K, N = 5, 3
    X = torch.eye(K).unsqueeze(0)
    W = (torch.arange(K).view(K, 1) + 100 * torch.arange(N).view(1, N))
    W = W.float().unsqueeze(0)
    want, _ = ref.grouped_linear_fwd_ref(X, W, torch.zeros(1, N), "linear")
    assert torch.equal(want[0], W[0].double())
    dX, _ = ref.grouped_linear_bwd_data_ref(X, W.transpose(1, 2).contiguous())
    assert torch.equal(dX[0], W[0].double())


@pytest.mark.parametrize("G,M,N,K", [(1, 1, 1, 1), (2, 11, 33, 7),
                                     (2, 70, 40, 65)])
def test_bwd_data_ref_vs_bmm_and_autograd(G, M, N, K):
    dZ, W = gc.rand(G, M, N, seed=4), gc.rand(G, K, N, seed=5)
    want, emu = ref.grouped_linear_bwd_data_ref(dZ, W)
    _close(want, torch.bmm(dZ.double(), W.double().transpose(1, 2)))
    # dX is the gradient of sum(dZ * (X @ W)) with respect to X
    X = torch.zeros(G, M, K, dtype=torch.float64, requires_grad=True)
    (torch.bmm(X, W.double()) * dZ.double()).sum().backward()
    _close(want, X.grad)
    assert emu.dtype == torch.float32


@pytest.mark.parametrize("G,M,K,N", [(1, 1, 1, 1), (3, 13, 24, 9)])
def test_gemm_acc_ref_vs_baddbmm(G, M, K, N):
    A, B = gc.rand(G, M, K, seed=8), gc.rand(G, K, N, seed=9)
    C0 = gc.rand(G, M, N, seed=10, scale=4.0)
    want, emu = ref.grouped_gemm_acc_ref(A, B, C0)
    _close(want, torch.baddbmm(C0.double(), A.double(), B.double()))
    assert emu.dtype == torch.float32


@pytest.mark.parametrize("act", gc.ACTS)
@pytest.mark.parametrize("l1", [0.0, 1e-4])
def test_act_l1_bwd_ref_vs_autograd(act, l1):
    """With Y = act(z): dZ is the gradient of sum(dA * Y) + l1 sum|Y|
    with respect to z (where z != 0 for relu)."""
    z = gc.rand_f32(4, 50, seed=11, scale=2.0).double()
    z[z == 0] = 0.5
    z.requires_grad_(True)
    Y = _act64(z, act)
    dA = gc.rand(4, 50, seed=12).double()
    l1f = float(torch.tensor(l1, dtype=torch.float32))
    ((dA * Y).sum() + l1f * Y.abs().sum()).backward()
    want, _ = ref.act_l1_bwd_ref(dA, Y.detach(), act, l1)
    _close(want, z.grad)


def test_act_l1_bwd_ref_zero_edges():
    Y = torch.tensor([0.0, -0.0, 0.5, -0.5])
    dA = torch.ones(4)
    for act in ("linear", "tanh", "sigmoid"):
        want, _ = ref.act_l1_bwd_ref(dA, Y, act, 1.0)
        d = ref.act_grad_from_output(Y.double(), ref.act_code(act))
        assert torch.equal(want, (dA.double() + torch.tensor(
            [0.0, 0.0, 1.0, -1.0], dtype=torch.float64)) * d)
    want, _ = ref.act_l1_bwd_ref(dA, Y, "relu", 1.0)
    assert want.tolist() == [0.0, 0.0, 2.0, 0.0]


@pytest.mark.parametrize("real_n", [-1, 77])
def test_mse_bwd_ref_vs_autograd(real_n):
    Y = gc.rand(2, 13, 9, seed=13).double().requires_grad_(True)
    T = gc.rand(2, 13, 9, seed=14).double()
    n = 13 * 9 if real_n <= 0 else real_n
    loss = ((Y - T) ** 2).sum(dim=(1, 2)) / n
    loss.sum().backward()
    (want_loss, want_dY), (emu_loss, emu_dY) = ref.mse_bwd_ref(
        Y.detach(), T, real_n
    )
    _close(want_loss, loss.detach())
    _close(want_dY, Y.grad)
    assert emu_loss.dtype == emu_dY.dtype == torch.float32
    assert (emu_loss.double() - want_loss).abs().max().item() < 1e-6


def test_lstm_pointwise_refs_vs_autograd():
    G, B, H = 2, 7, 5
    gates = gc.rand(G, B, 4 * H, seed=17, scale=3.0).double()
    gates.requires_grad_(True)
    c_prev = gc.rand_f32(G, B, H, seed=18).double().requires_grad_(True)
    (h, c, gact), (h32, c32, ga32) = ref.lstm_pointwise_fwd_ref(gates, c_prev)
    i, f, g, o = (
        torch.sigmoid(gates[..., 0:H]), torch.sigmoid(gates[..., H:2 * H]),
        torch.tanh(gates[..., 2 * H:3 * H]), torch.sigmoid(gates[..., 3 * H:]),
    )
    _close(c.detach(), (f * c_prev + i * g).detach())
    _close(h.detach(), (o * torch.tanh(f * c_prev + i * g)).detach())
    _close(gact.detach(), torch.cat([i, f, g, o], -1).detach())
    assert h32.dtype == c32.dtype == ga32.dtype == torch.float32
    # backward: gradient of sum(dh * h) + sum(dc_next * c)
    dh = gc.rand(G, B, H, seed=19).double()
    dc_next = gc.rand_f32(G, B, H, seed=20).double()
    ((dh * h).sum() + (dc_next * c).sum()).backward()
    (dg, dcp), (dg32, dcp32) = ref.lstm_pointwise_bwd_ref(
        dh, dc_next, gact.detach(), c.detach(), c_prev.detach()
    )
    _close(dg, gates.grad)
    _close(dcp, c_prev.grad)
    assert dg32.dtype == dcp32.dtype == torch.float32


def test_lstm_pointwise_fwd_ref_saturates():
    z = torch.tensor([30.0, 100.0, -30.0, -100.0])
    gates = torch.stack([z, z, z, z], dim=-1).reshape(1, 4, 4)  # H = 1
    (h, c, gact), _ = ref.lstm_pointwise_fwd_ref(gates, torch.ones(1, 4, 1))
    assert not torch.isnan(gact).any() and not torch.isnan(h).any()
    # rounded to bf16 the gates are exactly 0, 1 or -1 everywhere but
    # sigmoid(-30) = 9.36e-14, which bf16's exponent range still holds
    sig = gact.to(torch.bfloat16).float()[0, :, 0]
    assert sig[:2].tolist() == [1.0, 1.0] and sig[3].item() == 0.0
    assert sig[2].item() == pytest.approx(9.3576e-14, rel=2.0 ** -8)
    assert torch.equal(gact.to(torch.bfloat16).float()[0, :, 2],
                       torch.tensor([1.0, 1, -1, -1]))


def test_adam_step_ref_vs_keras_formula():
    n = 101
    p, g = gc.rand_f32(n, seed=15), gc.rand_f32(n, seed=16)
    m, v = gc.rand_f32(n, seed=21, scale=0.1), gc.rand_f32(n, seed=22).abs()
    lr, b1, b2, eps = (float(torch.tensor(x, dtype=torch.float32))
                       for x in (0.01, 0.9, 0.999, 1e-7))
    for step in (1, 2, 999):
        (p1, m1, v1), (p32, m32, v32) = ref.adam_step_ref(
            p, g, m, v, 0.01, 0.9, 0.999, 1e-7, step
        )
        pd, gd, md, vd = (t.double() for t in (p, g, m, v))
        wm = b1 * md + (1 - b1) * gd
        wv = b2 * vd + (1 - b2) * gd * gd
        mhat, vhat = wm / (1 - b1 ** step), wv / (1 - b2 ** step)
        _close(m1, wm)
        _close(v1, wv)
        _close(p1, pd - lr * mhat / (vhat.sqrt() + eps))
        assert p32.dtype == m32.dtype == v32.dtype == torch.float32
        assert (p32.double() - p1).abs().max().item() < 1e-5
    # the existing in-place fp32 reference agrees at fp32 precision
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    ref.adam_step(p2, g, m2, v2, 0.01, 0.9, 0.999, 1e-7, 2)
    (p1, m1, v1), _ = ref.adam_step_ref(p, g, m, v, 0.01, 0.9, 0.999, 1e-7, 2)
    assert (p2.double() - p1).abs().max().item() < 1e-6


def test_lattice_inputs_make_the_emulation_exact():
    """Ternary operands, integer bias in [-8, 8], K <= 128: every
    product and partial sum is an integer below 2^8, exact in fp32 and
    in bf16 — the premise of the zero-tolerance device tests."""
    G, M, K, N = 2, 9, 128, 11
    X, W = gc.ternary(G, M, K, seed=1), gc.ternary(G, K, N, seed=2)
    b = gc.integers(-8, 8, G, N, seed=3)
    want, emu = ref.grouped_linear_fwd_ref(X, W, b, "linear")
    assert want.abs().max().item() <= 136
    assert torch.equal(emu.double(), want)
    assert torch.equal(want.to(torch.bfloat16).double(), want)
    assert gc.emu_atol(want, emu) == 0.0


def test_bound_helpers_on_hand_made_cases():
    want = torch.tensor([1.0, -2.0, 0.0, 100.0], dtype=torch.float64)
    emu = want.float() + torch.tensor([0.0, 2.0 ** -20, 0.0, 0.0])
    atol = gc.emu_atol(want, emu)
    assert atol == 4 * 2.0 ** -20
    assert gc.emu_atol(want, emu, floor=1.0) == 1.0
    bound = gc.bf16_bound(want, atol)
    assert bound.tolist() == [2.0 ** -8 + atol, 2.0 ** -7 + atol, atol,
                              100 * 2.0 ** -8 + atol]
    f32b = gc.f32_bound(want, atol)
    assert f32b.tolist() == [atol, atol, atol, 100 * 2.0 ** -22]

    # half a bf16 ulp at 1 (2^-8) passes; one ulp (2^-7) does not
    one = torch.tensor([1.0], dtype=torch.float64)
    exact = one.float()
    gc.check_bf16("half ulp", torch.tensor([1.0 + 2.0 ** -7]).bfloat16(),
                  one + 2.0 ** -8, exact + 2.0 ** -8)
    with pytest.raises(AssertionError):
        gc.check_bf16("one ulp", torch.tensor([1.0 + 2.0 ** -7]).bfloat16(),
                      one, exact)
    # a NaN (an element the kernel never wrote) fails, it does not
    # compare as "not greater than the bound"
    with pytest.raises(AssertionError):
        gc.check_bf16("nan", torch.tensor([float("nan")]).bfloat16(),
                      one, exact)
    with pytest.raises(AssertionError):
        gc.check_f32("nan", torch.tensor([float("nan")]), one, exact)
    # fp32: 2 ulps of the output pass with an exact emulation, 2^-20 not
    gc.check_f32("2 ulp", torch.tensor([1.0 + 2.0 ** -22]), one, exact)
    with pytest.raises(AssertionError):
        gc.check_f32("far", torch.tensor([1.0 + 2.0 ** -20]), one, exact)
    # dtype is part of the contract
    with pytest.raises(AssertionError):
        gc.check_bf16("dtype", torch.tensor([1.0]), one, exact)


def test_case_tables_reach_their_arms():
    """The arithmetic the shape comments claim."""
    def nblocks(G, M, N):
        return G * -(-M // 64) * -(-N // 64)

    by = {s: nblocks(s[0], s[1], s[3]) for s in gc.FWD_SHAPES}
    assert by[(1, 65, 33, 65)] == 4          # below 8: no remap
    assert by[(1, 130, 50, 130)] % 8 == 1
    assert by[(5, 65, 24, 65)] % 8 == 4
    assert by[(4, 128, 64, 128)] % 8 == 0
    assert by[(9, 1, 7, 1)] == 9
    assert all(K <= 128 for _, _, K, _ in gc.FWD_SHAPES)
    assert all(s in gc.FWD_SHAPES for s in gc.PROP_SHAPES)
    assert len(gc.BWD_CASES) == 28 and len(gc.ACC_CASES) == 12
    assert all(n <= 128 for _, _, n, _ in gc.BWD_CASES)
