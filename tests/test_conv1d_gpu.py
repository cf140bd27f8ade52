"""The three grouped Conv1D kernels (csrc/conv1d.hip) against the fp64
oracles, over the case table of conv1d_cases.py.

Bounds are the project's (gemm_cases.py): a bf16 output keeps
|got - want| <= 2^-8 |want| + atol with atol = 4x the oracle's fp32
emulation error (floored at 2^-20 for the single-__expf tanh / sigmoid
epilogue), an fp32 output max(atol, 2^-22 |want|).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conv1d_cases import CASES, IDS, LATTICE_ROWS, NAN_ROW, reference
from gemm_cases import EXP_FLOOR, check_bf16, check_f32, ternary
from gordo_amd import ops


def _dev(t, dtype=torch.bfloat16):
    return t.to("cuda", dtype)


def _launched(entry, shape):
    G, B, T, Cin, Cout, k, d, padding, _act = shape
    plan = ops.conv1d_plan(entry, G, B, T, Cin, Cout, k, d, padding)
    assert plan is not None and ops.last_conv1d_launch() == plan
    return plan


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_kernels_against_the_oracle(i):
    assert ops.hip_available()
    shape, rows, resident, chunks, _what = CASES[i]
    G, B, T, Cin, Cout, k, d, padding, act = shape
    r = reference(i)
    x, W, dZ = _dev(r["x"]), _dev(r["W"]), _dev(r["dZ"])
    b = _dev(r["b"], torch.float32)

    y = ops.conv1d_fwd(x, W, b, act, padding, d)
    plan = _launched("fwd", shape)
    assert (plan["family"], plan["rows"], plan["taps_resident"]) == (
        "conv1d_fwd", rows, resident)
    check_bf16("fwd", y, *r["fwd"],
               floor=EXP_FLOOR if act in ("tanh", "sigmoid") else 0.0)
    # determinism: no atomics on this path
    assert torch.equal(ops.conv1d_fwd(x, W, b, act, padding, d), y)

    dX = ops.conv1d_bwd_data(dZ, W, padding, d)
    plan = _launched("bwd_data", shape)
    assert (plan["family"], plan["rows"], plan["taps_resident"]) == (
        "conv1d_bwd_data", rows, resident)
    check_bf16("bwd_data", dX, *r["bwd_data"])
    assert torch.equal(ops.conv1d_bwd_data(dZ, W, padding, d), dX)

    dW, db = ops.conv1d_wgrad(x, dZ, k, padding, d)
    plan = _launched("wgrad", shape)
    assert (plan["family"], plan["chunks"]) == ("conv1d_wgrad", chunks)
    (want_W, want_b), (emu_W, emu_b) = r["wgrad"]
    check_f32("dW", dW, want_W, emu_W)
    check_f32("db", db, want_b, emu_b)


@pytest.mark.parametrize("i", LATTICE_ROWS, ids=[IDS[i] for i in LATTICE_ROWS])
def test_wgrad_lattice_exact(i):
    """Ternary inputs: every partial sum is a small integer, so plain
    stores (one chunk) and fp32 atomics (two) must both be exact."""
    shape, _rows, _res, chunks, _what = CASES[i]
    G, B, T, Cin, Cout, k, d, padding, _act = shape
    x = ternary(G, B, T, Cin, seed=70 + i)
    dZ = ternary(G, B, T, Cout, seed=80 + i)
    dW, db = ops.conv1d_wgrad(_dev(x), _dev(dZ), k, padding, d)
    assert _launched("wgrad", shape)["chunks"] == chunks
    (want_W, want_b), _ = ops.reference.conv1d_wgrad_ref(x, dZ, k, padding, d)
    assert torch.equal(dW.cpu().double(), want_W)
    assert torch.equal(db.cpu().double(), want_b)


def test_nan_stays_in_its_window():
    """The edge zeros and the halo: a NaN in one window's input reaches
    that window's outputs and no other's, forward and bwd-data."""
    shape = CASES[NAN_ROW][0]
    G, B, T, Cin, Cout, k, d, padding, act = shape
    r = reference(NAN_ROW)
    W, b = _dev(r["W"]), _dev(r["b"], torch.float32)
    for name, clean_in, run in (
        ("fwd", r["x"], lambda t: ops.conv1d_fwd(t, W, b, act, padding, d)),
        ("bwd_data", r["dZ"],
         lambda t: ops.conv1d_bwd_data(t, W, padding, d)),
    ):
        clean = run(_dev(clean_in))
        bad_in = clean_in.clone()
        bad_in[1, 2, T // 2, 3] = float("nan")
        bad = run(_dev(bad_in))
        hit = torch.isnan(bad).flatten(2).any(dim=2).cpu()
        want = torch.zeros(G, B, dtype=torch.bool)
        want[1, 2] = True
        assert torch.equal(hit, want), name
        keep = ~want.to("cuda")
        assert torch.equal(bad[keep], clean[keep]), name
