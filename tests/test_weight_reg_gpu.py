"""The regularized optimizer step (opt_masked_kernel<KIND, true>) and
the per-model weight penalty (weight_penalty_*_kernel) of
masked_ops.hip against their fp64 oracles, on the segment tables of
test_masked_opt_gpu.py with coefficients mixed per segment.

Bounds: ``max(atol, 2^-22 |want|)`` with ``atol`` = 4x the error of the
oracle's own fp32 emulation (gemm_cases.check_f32); the lattice cases
allow no error at all."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_cases as gc
import regularizer_cases as rc
from gordo_amd import ops
from gordo_amd.engine.spec import resolve_optimizer
from gordo_amd.ops import reference as ref
from test_masked_opt_gpu import ARMS, ARM_IDS, MASKS, _State, _same

G = rc.KERNEL_G
NAMES = "p s0 s1 s2".split()
STEP_MASKS = {"unmasked": None, "alternating": MASKS["alternating"],
              "single": MASKS["single"], "none": MASKS["none"]}
MASKED_REG = {"family": "masked", "reg": True}


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def _mask(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def _setup(optimizer, kwargs, table_name, coeffs=None, shift=0):
    require_hip()
    kind, h = resolve_optimizer(optimizer, kwargs)
    sizes = rc.TABLES[table_name]
    offsets, n = rc.layout(sizes)
    table = ops.segment_table(offsets, sizes, "cuda")
    coeffs = rc.COEFFS[table_name] if coeffs is None else coeffs
    reg = ops.reg_table(*zip(*coeffs), "cuda")
    state = _State(n, h.get("initial_accumulator_value", 0.0), shift=shift)
    return kind, h, sizes, table, reg, state


def _step(state, kind, h, g, step, table, reg, active=None):
    ops.optimizer_step(
        kind, state.p, g, state.slots[0], state.slots[1], state.slots[2], h,
        step, state.lp, step_buf=state.step_buf, active=active,
        segments=table, reg=reg, G=G,
    )


@pytest.mark.parametrize("table_name", list(rc.TABLES))
@pytest.mark.parametrize("optimizer,kwargs", ARMS, ids=ARM_IDS)
def test_regularized_step_against_the_oracle(optimizer, kwargs, table_name):
    kind, h, sizes, table, reg, start = _setup(optimizer, kwargs, table_name)
    index = [rc.model_index(sizes, g) for g in range(G)]
    for mask_name, mask in STEP_MASKS.items():
        state = start.clone()
        live = [g for g in range(G) if mask is None or mask[g]]
        frozen = [g for g in range(G) if g not in live]
        for step, g_clean in enumerate(state.grads, 1):
            before = [t.cpu() for t in state.buffers()]
            grad = g_clean.clone()
            for g in frozen:  # never read: a NaN there changes nothing
                grad[index[g][::3].cuda()] = float("nan")
            g_seen = grad.clone()
            _step(state, kind, h, grad, step, table, reg,
                  None if mask is None else _mask(mask))
            assert ops.last_optimizer_launch() == MASKED_REG
            assert int(state.step_buf) == step
            assert _same(grad, g_seen)  # g32 is not modified
            want, emu = ref.reg_step_ref(
                kind, before[0], g_clean.cpu(), *before[1:4], h, step,
                table, reg, G)
            got = [t.cpu() for t in state.buffers()]
            if live:
                idx = torch.cat([index[g] for g in live])
                for name, gt, wt, em in zip(NAMES, got, want, emu):
                    gc.check_f32(f"{mask_name} step {step} {name}",
                                 gt[idx], wt[idx], em[idx])
                # the mirror is the kernel's own p, rounded
                assert _same(got[4][idx], got[0][idx].to(torch.bfloat16))
            for g in frozen:
                for name, gt, was in zip(NAMES + ["lp"], got, before):
                    assert _same(gt[index[g]], was[index[g]]), (
                        mask_name, step, name, g)
        if live:
            # the term is there: the plain step ends elsewhere
            plain = start.clone()
            for step, g_clean in enumerate(plain.grads, 1):
                plain.step(kind, h, g_clean, step)
            seg = rc.segment_index(sizes, len(sizes) - 1).cuda()
            coeff = rc.COEFFS[table_name][-1]
            assert _same(plain.p[seg], state.p[seg]) == (
                coeff == (0.0, 0.0) and mask is None)


@pytest.mark.parametrize("table_name", list(rc.TABLES))
def test_regularized_sgd_on_a_lattice_is_exact(table_name):
    """lr = 2^-2, l1 = 2^-3, l2 = 2^-4, p in {-1, -0.5, -0, 0, 0.5, 1}
    and g in multiples of 2^-4: every product and sum is exact."""
    sizes = rc.TABLES[table_name]
    kind, h, _s, table, reg, state = _setup(
        "SGD", {"learning_rate": 0.25}, table_name,
        coeffs=[(0.125, 0.0625)] * len(sizes))
    n = state.p.numel()
    gen = torch.Generator().manual_seed(31)
    values = torch.tensor([-1.0, -0.5, -0.0, 0.0, 0.5, 1.0])
    p = values[torch.randint(0, 6, (n,), generator=gen)]
    g = torch.randint(-32, 33, (n,), generator=gen).float() / 16
    zero = (p == 0) & (torch.rand(n, generator=gen) < 0.5)
    g[zero] = 0.0
    assert int(zero.sum()) > 10 and bool((p[zero].signbit()).any())
    state.p.copy_(p)
    state.lp.copy_(p)
    _step(state, kind, h, g.cuda(), 1, table, reg)
    (want, *_), (emu, *_) = ref.reg_step_ref(
        kind, p, g, None, None, None, h, 1, table, reg, G)
    assert torch.equal(want, emu.double())  # exact in fp32 too
    assert _same(state.p.cpu(), want.float())
    assert _same(state.lp.cpu(), want.to(torch.bfloat16))
    assert bool((state.p.cpu()[zero] == 0).all())
    assert not torch.equal(want.float(), p - 0.25 * g)
    assert ops.last_optimizer_launch() == MASKED_REG


@pytest.mark.parametrize("optimizer,kwargs", ARMS, ids=ARM_IDS)
def test_zero_coefficient_segments_take_the_plain_masked_step(optimizer,
                                                              kwargs):
    for table_name, sizes in rc.TABLES.items():
        kind, h, _s, table, reg, reg_state = _setup(optimizer, kwargs,
                                                    table_name)
        zero_state, plain = reg_state.clone(), reg_state.clone()
        zero_reg = torch.zeros_like(reg)
        active = _mask([1] * G)
        for step, g in enumerate(reg_state.grads, 1):
            plain.step(kind, h, g, step, active, table)
            assert ops.last_optimizer_launch() == {"family": "masked",
                                                   "reg": False}
            _step(zero_state, kind, h, g, step, table, zero_reg, active)
            _step(reg_state, kind, h, g, step, table, reg, active)
            assert ops.last_optimizer_launch() == MASKED_REG
        for name, a, z, b in zip(NAMES + ["lp"], reg_state.buffers(),
                                 zero_state.buffers(), plain.buffers()):
            assert _same(z, b), (table_name, name)
            for s, coeff in enumerate(rc.COEFFS[table_name]):
                seg = rc.segment_index(sizes, s).cuda()
                if coeff == (0.0, 0.0):
                    assert _same(a[seg], b[seg]), (table_name, name, s)
                elif name == "p":
                    assert not _same(a[seg], b[seg]), (table_name, name, s)


@pytest.mark.parametrize("table_name", ["aligned", "odd"])
def test_misaligned_buffers_give_the_same_bits(table_name):
    _k, _h, _s, table, reg, base = _setup("Adam", {}, table_name)
    kind, h, _s, _t, _r, moved = _setup("Adam", {}, table_name, shift=1)
    assert moved.p.data_ptr() % 16 == 4 and base.p.data_ptr() % 16 == 0
    assert _same(moved.p, base.p)
    for step, g in enumerate(base.grads, 1):
        _step(base, kind, h, g, step, table, reg, _mask(MASKS["alternating"]))
        _step(moved, kind, h, moved.grads[step - 1], step, table, reg,
              _mask(MASKS["alternating"]))
    for a, b in zip(base.buffers(), moved.buffers()):
        assert _same(a, b)
    assert _same(ops.weight_penalty(base.p, table, reg, G),
                 ops.weight_penalty(moved.p, table, reg, G))


def _penalty_case(table_name):
    require_hip()
    sizes = rc.TABLES[table_name]
    offsets, n = rc.layout(sizes)
    table = ops.segment_table(offsets, sizes, "cuda")
    reg = ops.reg_table(*zip(*rc.COEFFS[table_name]), "cuda")
    return sizes, n, table, reg


@pytest.mark.parametrize("table_name", list(rc.TABLES))
def test_penalty_on_a_lattice_is_exact(table_name):
    """p in multiples of 2^-3, |p| <= 1, coefficients powers of two:
    every sum is exact in fp32, in any order."""
    _sizes, n, table, reg = _penalty_case(table_name)
    gen = torch.Generator().manual_seed(41)
    p = torch.randint(-8, 9, (n,), generator=gen).float() / 8
    want, emu = ref.weight_penalty_ref(p, table, reg, G)
    assert torch.equal(want, emu.double()) and bool((want > 0).all())
    pd = p.cuda()
    got = ops.weight_penalty(pd, table, reg, G)
    assert got.dtype == torch.float32 and tuple(got.shape) == (G,)
    assert _same(got.cpu(), want.float())
    assert _same(pd.cpu(), p)  # p is only read
    # the CPU op agrees
    assert torch.equal(ops.weight_penalty(p, table.cpu(), reg.cpu(), G),
                       want.float())


@pytest.mark.parametrize("table_name", list(rc.TABLES))
def test_penalty_of_random_weights_against_the_oracle(table_name):
    _sizes, n, table, reg = _penalty_case(table_name)
    p = gc.rand_f32(n, seed=43)
    want, emu = ref.weight_penalty_ref(p, table, reg, G)
    got = ops.weight_penalty(p.cuda(), table, reg, G)
    gc.check_f32(f"penalty {table_name}", got, want, emu)
    # an all-zero table is no penalty
    assert bool((ops.weight_penalty(p.cuda(), table, torch.zeros_like(reg),
                                    G) == 0).all())


@pytest.mark.parametrize("per", [(3, 8), (8, 64, 264, 4104)])
def test_penalty_bits_do_not_depend_on_the_layout(per):
    """One model's values as model 2 of a G = 4 buffer and as model 0
    of a G = 3 one. With per = (3, 8) the size-8 tensor starts at 12 +
    2 * 8 = 28 in the first (16-byte vectors) and at 9 in the second
    (element-wise)."""
    require_hip()
    gen = torch.Generator().manual_seed(47)
    values = [torch.rand(n, generator=gen) * 2 - 1 for n in per]
    coeffs = [(0.3, 0.7)] * len(per)
    results = []
    for G_, slot in ((4, 2), (3, 0)):
        offsets, n = rc.layout(per, G_)
        if per == (3, 8):
            assert (offsets[1] + slot * 8) % 4 == (0 if G_ == 4 else 1)
        p = torch.rand(n, generator=gen) * 2 - 1
        for off, size, v in zip(offsets, per, values):
            p[off + slot * size: off + (slot + 1) * size] = v
        table = ops.segment_table(offsets, per, "cuda")
        reg = ops.reg_table(*zip(*coeffs), "cuda")
        pd = p.cuda()
        first = ops.weight_penalty(pd, table, reg, G_)
        again = ops.weight_penalty(pd, table, reg, G_)
        assert _same(first, again)  # the same on every launch
        want, emu = ref.weight_penalty_ref(p, table, reg, G_)
        gc.check_f32(f"penalty G={G_}", first, want, emu)
        results.append(first[slot].reshape(1).cpu())
    assert _same(results[0], results[1])


def test_bad_table_entries_are_skipped_by_the_regularized_ops():
    require_hip()
    sizes = (8, 16)
    offsets, n = rc.layout(sizes)
    good = ops.segment_table(offsets, sizes, "cuda")
    bad = ops.segment_table(
        offsets + [n - 8, -4, 0], list(sizes) + [16, 8, n], "cuda")
    good_reg = ops.reg_table([0.5, 0.25], [0.125, 0.0], "cuda")
    bad_reg = ops.reg_table([0.5, 0.25, 1, 1, 1], [0.125, 0.0, 1, 1, 1],
                            "cuda")
    p = gc.rand_f32(n, seed=53).cuda()
    assert _same(ops.weight_penalty(p, good, good_reg, G),
                 ops.weight_penalty(p, bad, bad_reg, G))
    h = resolve_optimizer("SGD", {})[1]
    g = gc.rand_f32(n, seed=54).cuda()
    step_buf = torch.zeros(1, dtype=torch.int32, device="cuda")
    a, b = p.clone(), p.clone()
    ops.optimizer_step("sgd", a, g, None, None, None, h, 1,
                       step_buf=step_buf, segments=good, reg=good_reg, G=G)
    ops.optimizer_step("sgd", b, g, None, None, None, h, 1,
                       step_buf=step_buf, segments=bad, reg=bad_reg, G=G)
    assert _same(a, b) and not _same(a, p)


def test_launch_record_and_argument_checks():
    kind, h, _s, table, reg, state = _setup("Adam", {}, "aligned")
    state.step(kind, h, state.grads[0], 1)
    assert ops.last_optimizer_launch() == {"family": "adam", "reg": False}
    sgd_kind, sgd_h = resolve_optimizer("SGD", {})
    state.step(sgd_kind, sgd_h, state.grads[0], 2)
    assert ops.last_optimizer_launch() == {"family": "opt", "reg": False}
    _step(state, kind, h, state.grads[0], 3, table, reg)
    assert ops.last_optimizer_launch() == MASKED_REG
    with pytest.raises(ValueError, match="segment table"):
        ops.optimizer_step(kind, state.p, state.grads[0], *state.slots, h, 4,
                           state.lp, step_buf=state.step_buf, reg=reg, G=G)
    with pytest.raises(ValueError, match="active or G"):
        ops.optimizer_step(kind, state.p, state.grads[0], *state.slots, h, 4,
                           state.lp, step_buf=state.step_buf, segments=table,
                           reg=reg)
    with pytest.raises(RuntimeError):  # S of the two tables differs
        _step(state, kind, h, state.grads[0], 4, table, reg[:, :2].contiguous())
    with pytest.raises(RuntimeError):
        ops.weight_penalty(state.p, table, reg.double(), G)
