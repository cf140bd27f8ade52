"""The 16-byte pipelined LSTM backward scan against the kernels it
replaces (lstm_seq_bwd_v5_kernel / lstm_seq_bwd_v3_kernel).

The new kernel changes how the per-step tile moves (16-byte loads into
an LDS ring, 16-byte stores from LDS) and nothing about the arithmetic,
so the bar is bit-equality with ``GORDO_LSTM_PIPE=0``; an fp32 CPU
oracle, repeat-launch determinism and guard-region checks cover what
bit-equality to a sibling kernel cannot.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops

ROW_TILES = ["16", "32", "64"]

# (G, B, T, H, F)
SHAPES = [
    (1, 1, 1, 8, 8),
    (1, 17, 2, 8, 8),        # T below the prefetch depth, one live row
    (2, 33, 3, 16, 16),
    (2, 48, 16, 48, 56),     # bench dims
    (2, 40, 12, 40, 48),
    (1, 33, 10, 32, 40),
    (2, 40, 12, 64, 128),    # caps: the LDS budget halves the row tile
]


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def to_dev_bf16(t):
    return t.to("cuda", torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _case(G, B, T, H, F):
    """One training forward per shape, shared (read-only) by every test:
    (Wx, Wh, cs, gacts, dSeq[last_only], dSeq[full])."""
    x = to_dev_bf16(_rand(G, B, T, F, seed=95) * 0.5)
    Wx = to_dev_bf16(_rand(G, F, 4 * H, seed=96) * 0.2)
    Wh = to_dev_bf16(_rand(G, H, 4 * H, seed=97) * 0.2)
    b = _rand(G, 4 * H, seed=98).cuda() * 0.1
    _, cs, ga = ops.lstm_seq_fwd_fused(x, Wx, Wh, b, store_aux=True)
    d_last = to_dev_bf16(_rand(G, B, H, seed=99))
    d_full = to_dev_bf16(_rand(G, B, T, H, seed=99))
    return Wx, Wh, cs, ga, d_last, d_full


def _run_both(fn, monkeypatch):
    """fn() under GORDO_LSTM_PIPE=0 (old kernels) and the default."""
    monkeypatch.setenv("GORDO_LSTM_PIPE", "0")
    old = fn()
    monkeypatch.delenv("GORDO_LSTM_PIPE")
    new = fn()
    return old, new


@pytest.mark.parametrize("rows", ROW_TILES)
@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("G,B,T,H,F", SHAPES)
def test_pipe_bwd_bit_equal_to_old(G, B, T, H, F, last_only, rows,
                                   monkeypatch):
    """dG, dX of lstm_seq_bwd_fused and dG of lstm_seq_bwd_v3 are
    bit-identical with the switch off and on."""
    require_hip()
    monkeypatch.setenv("GORDO_LSTM_ROWS", rows)
    Wx, Wh, cs, ga, d_last, d_full = _case(G, B, T, H, F)
    dSeq = d_last if last_only else d_full
    (dG0, dX0), (dG1, dX1) = _run_both(
        lambda: ops.lstm_seq_bwd_fused(dSeq, ga, cs, Wh, Wx, last_only),
        monkeypatch,
    )
    assert torch.equal(dG0, dG1)
    assert torch.equal(dX0, dX1)
    b0, b1 = _run_both(
        lambda: ops.lstm_seq_bwd_v3(dSeq, ga, cs, Wh, last_only),
        monkeypatch,
    )
    assert torch.equal(b0, b1)


def _oracle_bwd(dSeq, ga, cs, Wh, Wx, last_only):
    """fp32 CPU reverse scan. The scan entry points have no CPU path of
    their own, so the oracle steps the CPU fp32 paths of the ops they
    fuse: lstm_pointwise_bwd per step, bmm for the carry, and
    grouped_linear_bwd_data for dX."""
    ga, cs, Wh, Wx, dSeq = (
        t.float().cpu() for t in (ga, cs, Wh, Wx, dSeq)
    )
    G, B, T, H4 = ga.shape
    H = H4 // 4
    dG = torch.empty(G, B, T, H4)
    dh_carry = torch.zeros(G, B, H)
    dc = torch.zeros(G, B, H)
    for t in range(T - 1, -1, -1):
        dh = dh_carry.clone()
        if not last_only:
            dh += dSeq[:, :, t]
        elif t == T - 1:
            dh += dSeq
        c_prev = cs[:, :, t - 1] if t > 0 else torch.zeros(G, B, H)
        dg, dc = ops.lstm_pointwise_bwd(dh, dc, ga[:, :, t], cs[:, :, t],
                                        c_prev)
        dG[:, :, t] = dg
        dh_carry = torch.bmm(dg, Wh.transpose(1, 2))
    dX = ops.grouped_linear_bwd_data(dG.view(G, B * T, H4), Wx).view(
        G, B, T, Wx.shape[1]
    )
    return dG, dX


@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("G,B,T,H,F", [(2, 48, 16, 48, 56),
                                       (1, 33, 10, 16, 16)])
def test_pipe_bwd_matches_cpu_oracle(G, B, T, H, F, last_only):
    """The new path against the fp32 CPU oracle at the tolerances of
    test_lstm_seq_bwd_v5_fused_dseq."""
    require_hip()
    Wx, Wh, cs, ga, d_last, d_full = _case(G, B, T, H, F)
    dSeq = d_last if last_only else d_full
    want_dG, want_dX = _oracle_bwd(dSeq, ga, cs, Wh, Wx, last_only)
    dG, dX = ops.lstm_seq_bwd_fused(dSeq, ga, cs, Wh, Wx, last_only)
    dGb = ops.lstm_seq_bwd_v3(dSeq, ga, cs, Wh, last_only)
    for name, got, want in (("dG", dG, want_dG), ("dX", dX, want_dX),
                            ("dG bottom", dGb, want_dG)):
        err = (got.float().cpu() - want).abs().max().item()
        print(f"{name}: max abs err {err:.3e}, scale "
              f"{want.abs().max().item():.3e}")
    torch.testing.assert_close(dG.float().cpu(), want_dG, rtol=3e-2,
                               atol=1e-2)
    torch.testing.assert_close(dGb.float().cpu(), want_dG, rtol=3e-2,
                               atol=1e-2)
    torch.testing.assert_close(dX.float().cpu(), want_dX, rtol=5e-2,
                               atol=2e-2)


@pytest.mark.parametrize("last_only", [True, False])
def test_pipe_h_not_multiple_of_8_keeps_old_kernel(last_only, monkeypatch):
    """H = 42 has no 16-byte rows: both entry points still run the old
    kernels and give the same bits under either switch value."""
    require_hip()
    G, B, T, H, F = 2, 20, 6, 42, 50
    xW = to_dev_bf16(_rand(G, B, T, 4 * H, seed=50))
    Wh = to_dev_bf16(_rand(G, H, 4 * H, seed=51) * 0.2)
    Wx = to_dev_bf16(_rand(G, F, 4 * H, seed=53) * 0.2)
    _, cs, ga = ops.lstm_seq_fwd(xW, Wh)
    dSeq = to_dev_bf16(
        _rand(G, B, H, seed=52) if last_only else _rand(G, B, T, H, seed=52)
    )
    b0, b1 = _run_both(
        lambda: ops.lstm_seq_bwd_v3(dSeq, ga, cs, Wh, last_only),
        monkeypatch,
    )
    assert torch.equal(b0, b1)
    (dG0, dX0), (dG1, dX1) = _run_both(
        lambda: ops.lstm_seq_bwd_fused(dSeq, ga, cs, Wh, Wx, last_only),
        monkeypatch,
    )
    assert torch.equal(dG0, dG1)
    assert torch.equal(dX0, dX1)
    # and the old kernels agree with each other, as before
    assert torch.equal(b1, dG1)


@pytest.mark.parametrize("rows", ROW_TILES)
@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("G,B,T,H,F", [(2, 64, 24, 64, 128),
                                       (2, 64, 16, 48, 56)])
def test_pipe_bwd_deterministic(G, B, T, H, F, last_only, rows,
                                monkeypatch):
    """Five repeated launches of the new backward are bitwise identical
    (an LDS ring or staging race would show up as run-to-run drift)."""
    require_hip()
    monkeypatch.setenv("GORDO_LSTM_ROWS", rows)
    monkeypatch.delenv("GORDO_LSTM_PIPE", raising=False)
    Wx, Wh, cs, ga, d_last, d_full = _case(G, B, T, H, F)
    dSeq = d_last if last_only else d_full
    ref_dG, ref_dX = ops.lstm_seq_bwd_fused(dSeq, ga, cs, Wh, Wx, last_only)
    ref_b = ops.lstm_seq_bwd_v3(dSeq, ga, cs, Wh, last_only)
    for _ in range(5):
        dG, dX = ops.lstm_seq_bwd_fused(dSeq, ga, cs, Wh, Wx, last_only)
        assert torch.equal(dG, ref_dG)
        assert torch.equal(dX, ref_dX)
        assert torch.equal(
            ops.lstm_seq_bwd_v3(dSeq, ga, cs, Wh, last_only), ref_b
        )


GUARD = 4096            # bf16 elements on each side (16-byte aligned)
POISON = -12345.0


def _guarded(shape):
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((GUARD + n + GUARD,), POISON, dtype=torch.bfloat16,
                     device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == POISON).all()) and bool(
        (buf[-GUARD:] == POISON).all()
    )


@pytest.mark.parametrize("rows", ROW_TILES)
@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("G,B,T,H,F", [(1, 17, 2, 8, 8),
                                       (2, 33, 3, 16, 16),
                                       (1, 33, 10, 32, 40)])
def test_pipe_bwd_stays_in_bounds(G, B, T, H, F, last_only, rows,
                                  monkeypatch):
    """Ragged row tiles (B = 17, 33): with dG and dX placed inside a
    poisoned buffer, the 16-byte stores fill exactly the outputs and
    leave the guard regions on both sides untouched."""
    require_hip()
    monkeypatch.setenv("GORDO_LSTM_ROWS", rows)
    monkeypatch.delenv("GORDO_LSTM_PIPE", raising=False)
    Wx, Wh, cs, ga, d_last, d_full = _case(G, B, T, H, F)
    dSeq = d_last if last_only else d_full
    want_dG, want_dX = ops.lstm_seq_bwd_fused(dSeq, ga, cs, Wh, Wx,
                                              last_only)
    gbuf, dG = _guarded((G, B, T, 4 * H))
    xbuf, dX = _guarded((G, B, T, F))
    ops.lstm_seq_bwd_fused_out(dSeq, ga, cs, Wh, Wx, last_only, dG, dX)
    assert _guards_intact(gbuf) and _guards_intact(xbuf)
    assert torch.equal(dG, want_dG)
    assert torch.equal(dX, want_dX)
    bbuf, dGb = _guarded((G, B, T, 4 * H))
    ops.lstm_seq_bwd_v3_out(dSeq, ga, cs, Wh, last_only, dGb)
    assert _guards_intact(bbuf)
    assert torch.equal(dGb, want_dG)
