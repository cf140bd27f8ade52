"""Case tables, input builders and the error bounds for the grouped
GEMM and pointwise training kernels, shared by the CPU oracle
validation (test_gemm_oracle.py) and the device tests
(test_gemm_kernels_gpu.py, test_ops_gpu.py).

The bounds are derived, not tuned (docs/kernels.md, "Grouped GEMM arms"):

* A bf16 output is the round-to-nearest of an fp32 pre-image. Rounding
  costs at most half a bf16 ulp, which is <= 2^-8 |want| for normal
  values; the pre-image's own fp32 error is bounded by ``atol`` = 4x
  the largest error of the same computation done in fp32 on the CPU
  (the oracles' "emulation"). So ``|got - want| <= 2^-8 |want| + atol``.
* An fp32 output must keep ``max(atol, 2^-22 |want|)``: the same 4x
  emulation error, floored at 2 ulps of the output.
* The single-``__expf`` tanh and sigmoid carry a few fp32 ulps of 1 in
  absolute terms that no CPU emulation reproduces: for them ``atol`` is
  floored at 2^-20.
"""
import torch

ACTS = ("linear", "tanh", "relu", "sigmoid")
EXP_FLOOR = 2.0 ** -20

# grouped_linear_fwd (G, M, K, N): one row per arm of grouped_gemm_kernel,
# the smallest shape that reaches it. all_acts: every activation runs.
FWD_CASES = [
    # (G, M, K, N), all_acts, what it reaches
    ((1, 1, 1, 1), False, "smallest"),
    ((1, 64, 32, 64), True, "one tile, one k-step, 16-byte A"),
    ((1, 65, 33, 65), True, "one past every edge, scalar A, 4 blocks"),
    ((3, 63, 31, 63), False, "one short of every edge"),
    ((2, 70, 8, 70), False, "one 16-byte slice, three wholly past K"),
    ((2, 70, 40, 70), True, "K%8==0, K%32!=0, two k-steps"),
    ((2, 70, 72, 10), False, "three k-steps, narrow N"),
    ((1, 130, 50, 130), False, "9 blocks: remap r=1"),
    ((5, 65, 24, 65), False, "20 blocks: remap r=4, several groups"),
    ((4, 128, 64, 128), False, "16 blocks: remap r=0"),
    ((9, 1, 7, 1), False, "remap with 1x1 tiles"),
]
FWD_SHAPES = [c[0] for c in FWD_CASES]
FWD_ACT_CASES = [
    (shape, act)
    for shape, all_acts, _ in FWD_CASES
    for act in (ACTS if all_acts else ("linear",))
]
# the rows the further properties (poison, NaN containment, offset
# views) run on
PROP_SHAPES = [(2, 70, 40, 70), (1, 130, 50, 130)]

# grouped_linear_bwd_data (G, M, inner, K_out): both B staging forms
# (inner % 8 == 0 or not) and their tails
BWD_G, BWD_M = 2, 70
BWD_INNER = (1, 7, 8, 33, 40, 64, 72)
BWD_KOUT = (1, 63, 65, 130)
BWD_CASES = [(BWD_G, BWD_M, n, k) for n in BWD_INNER for k in BWD_KOUT]

ACC_K = (1, 8, 24, 33, 40, 72)
ACC_CASES = [(3, 65, k, 96) for k in ACC_K] + [(1, 1, k, 1) for k in ACC_K]

# the arm shapes of test_grouped_linear_wgrad_arms_vs_fp64, plus the
# big-M row (M = 4177: split-M with a ragged last chunk)
WGRAD_CASES = [
    (2, 20, 50, 38),
    (1, 32, 8, 8),
    (1100, 40, 8, 8),
    (2, 200, 72, 38),
    (1, 100, 130, 70),
    (1, 4177, 50, 38),
]
# grouped_wgrad_xh / _hprev (G, B, T, F, H)
WGRAD_XH_CASES = [(2, 4, 5, 34, 16), (1, 10, 10, 66, 64), (1, 29, 144, 8, 8)]

# grid-stride launch caps (gordo_kernels.hip launchers): one element
# count past each forces a second trip of the loop
CAP_POINTWISE = 2048 * 256
CAP_MSE = 512 * 256
CAP_ADAM = 4096 * 256


def bf16r(t):
    """Round to bf16 and back: the kernel's view of an operand."""
    return t.to(torch.bfloat16).to(torch.float32)


def rand(*shape, seed=0, scale=1.0):
    """Uniform in [-scale, scale), already rounded to bf16 (fp32)."""
    g = torch.Generator().manual_seed(seed)
    return bf16r((torch.rand(*shape, generator=g) * 2 - 1) * scale)


def rand_f32(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def ternary(*shape, seed=0):
    """Values drawn from {-1, 0, 1}."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, shape, generator=g).to(torch.float32)


def integers(lo, hi, *shape, seed=0):
    """Integers in [lo, hi] as fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


def emu_atol(want, emu, floor=0.0):
    """4x the largest error of the fp32 emulation, floored."""
    return max(4.0 * (emu.double() - want).abs().max().item(), floor)


def bf16_bound(want, atol):
    return 2.0 ** -8 * want.abs() + atol


def f32_bound(want, atol):
    return torch.clamp(2.0 ** -22 * want.abs(), min=atol)


def _report(name, got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    # NaN in got (an unwritten, poisoned element) must fail: compare
    # through ~(err <= bound)
    bad = ~(err <= bound)
    excess = (err - 2.0 ** -8 * want.abs()).max().item()
    print(f"{name}: max abs err {err.max().item():.3e}, {what}, "
          f"scale {want.abs().max().item():.3e}, "
          f"max(err - 2^-8|want|) {excess:.3e}")
    assert not bool(bad.any()), (
        f"{name}: {int(bad.sum())} elements beyond the bound ({what}); "
        f"worst err {err[bad].max().item():.3e} at flat index "
        f"{int(bad.flatten().nonzero()[0])}"
    )
    return excess


def check_bf16(name, got, want, emu, floor=0.0):
    """|got - want| <= 2^-8 |want| + atol for a bf16 kernel output.
    Returns max(|got - want| - 2^-8 |want|), the part ``atol`` has to
    cover."""
    assert got.dtype == torch.bfloat16, got.dtype
    assert tuple(got.shape) == tuple(want.shape)
    atol = emu_atol(want, emu, floor)
    return _report(name, got, want, bf16_bound(want, atol),
                   f"atol {atol:.3e}")


def check_f32(name, got, want, emu, floor=0.0):
    """|got - want| <= max(atol, 2^-22 |want|) for an fp32 output."""
    assert got.dtype == torch.float32, got.dtype
    assert tuple(got.shape) == tuple(want.shape)
    atol = emu_atol(want, emu, floor)
    return _report(name, got, want, f32_bound(want, atol),
                   f"atol {atol:.3e}")


def wgrad_oracle(A, dZ):
    """fp64 bmm on the bf16-rounded inputs, and the bound the kernel's
    fp32 result must keep against it: 4x the error of the same product
    in fp32 on the CPU, floored at 2 ulps of the fp32 output."""
    A, dZ = (t.to(torch.bfloat16).double() for t in (A, dZ))
    want_W = torch.bmm(A.transpose(1, 2), dZ)
    want_b = dZ.sum(dim=1)
    emu_W = torch.bmm(A.float().transpose(1, 2), dZ.float())
    emu_b = dZ.float().sum(dim=1)
    atol_W = 4 * (emu_W.double() - want_W).abs().max().item()
    atol_b = 4 * (emu_b.double() - want_b).abs().max().item()
    return (want_W, atol_W), (want_b, atol_b)


def check_wgrad(name, got, want_atol):
    want, atol = want_atol
    assert got.dtype == torch.float32
    err = (got.double().cpu() - want).abs()
    bound = torch.clamp(2.0 ** -22 * want.abs(), min=atol)
    print(f"{name}: max abs err {err.max().item():.3e}, atol {atol:.3e}, "
          f"scale {want.abs().max().item():.3e}")
    assert bool((err <= bound).all()), (
        f"{name}: max err {err.max().item():.3e} beyond "
        f"max({atol:.3e}, 2^-22 |want|)"
    )
