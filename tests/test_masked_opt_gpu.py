"""The masked optimizer step and the masked copy (masked_ops.hip):
bit-equal to the unmasked kernels for the active models, and no touch
at all of the frozen ones."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops
from gordo_amd.engine.spec import resolve_optimizer

G = 5
# per-model sizes of the S tensors of a flat buffer
TABLES = {
    # offsets 0, 5, 40, 80, 245: misaligned bases, odd sizes; only the
    # size-8 tensor (base 40 + 8g) can move as 16-byte vectors
    "odd": (1, 7, 8, 33, 264),
    # every size a multiple of 8, every base 16-byte aligned; 4440
    # elements per model: several blocks per model
    "aligned": (8, 64, 264, 4104),
    # element-wise with several blocks per model
    "odd_large": (3, 2051, 1030),
}
ARMS = [
    ("Adam", {"learning_rate": 0.01}),
    ("Adam", {"amsgrad": True, "learning_rate": 0.01}),
    ("SGD", {}),
    ("SGD", {"momentum": 0.9}),
    ("SGD", {"momentum": 0.9, "nesterov": True}),
    ("RMSprop", {}),
    ("RMSprop", {"momentum": 0.8, "rho": 0.95}),
    ("Adagrad", {}),
    ("Adamax", {"learning_rate": 0.002}),
]
ARM_IDS = ["adam", "adam-amsgrad", "sgd", "sgd-momentum", "sgd-nesterov",
           "rmsprop", "rmsprop-momentum", "adagrad", "adamax"]
MASKS = {
    "first": [1, 0, 0, 0, 0],
    "last": [0, 0, 0, 0, 1],
    "alternating": [1, 0, 1, 0, 1],
    "single": [0, 0, 1, 0, 0],
    "none": [0, 0, 0, 0, 0],
}


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def _layout(sizes):
    offsets, total = [], 0
    for per in sizes:
        offsets.append(total)
        total += G * per
    return offsets, total


def _model_index(sizes, g):
    """Flat indices of model g's elements."""
    offsets, _ = _layout(sizes)
    return torch.cat([
        torch.arange(off + g * per, off + (g + 1) * per)
        for off, per in zip(offsets, sizes)
    ]).cuda()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class _State:
    """p, the three slots, the bf16 mirror and the step counter."""

    def __init__(self, n, init0, seed=15, shift=0):
        gen = torch.Generator().manual_seed(seed)

        def dev(t):
            # shift > 0 moves every buffer off its 16-byte alignment
            buf = torch.empty(n + shift, dtype=t.dtype, device="cuda")
            buf[shift:].copy_(t)
            return buf[shift:]

        self._dev = dev
        self.p = dev(torch.rand(n, generator=gen) * 2 - 1)
        self.slots = [dev(torch.full((n,), float(init0))),
                      dev(torch.zeros(n)), dev(torch.zeros(n))]
        self.lp = dev(self.p.to(torch.bfloat16))
        self.step_buf = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.grads = [
            dev((torch.rand(n, generator=gen) * 2 - 1) / t ** 2)
            for t in (1, 2, 3)
        ]

    def clone(self):
        other = object.__new__(_State)
        other._dev = self._dev
        other.p = self._dev(self.p)
        other.slots = [self._dev(s) for s in self.slots]
        other.lp = self._dev(self.lp)
        other.step_buf = self.step_buf.clone()
        other.grads = self.grads
        return other

    def buffers(self):
        return [self.p, *self.slots, self.lp]

    def step(self, kind, h, g, step, active=None, table=None):
        ops.optimizer_step(
            kind, self.p, g, self.slots[0], self.slots[1], self.slots[2], h,
            step, self.lp, step_buf=self.step_buf, active=active,
            segments=table,
        )


def _setup(optimizer, kwargs, table_name, shift=0):
    require_hip()
    kind, h = resolve_optimizer(optimizer, kwargs)
    sizes = TABLES[table_name]
    offsets, n = _layout(sizes)
    table = ops.segment_table(offsets, sizes, "cuda")
    state = _State(n, h.get("initial_accumulator_value", 0.0), shift=shift)
    return kind, h, sizes, table, state


def _mask(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("table_name", list(TABLES))
@pytest.mark.parametrize("optimizer,kwargs", ARMS, ids=ARM_IDS)
def test_all_active_is_bitwise_the_unmasked_step(optimizer, kwargs,
                                                 table_name):
    kind, h, _sizes, table, masked = _setup(optimizer, kwargs, table_name)
    plain = masked.clone()
    active = _mask([1] * G)
    for step, g in enumerate(masked.grads, 1):
        plain.step(kind, h, g, step)
        masked.step(kind, h, g, step, active, table)
        for name, a, b in zip("p s0 s1 s2 lp".split(), masked.buffers(),
                              plain.buffers()):
            assert _same(a, b), (name, step)
    assert int(masked.step_buf) == 3 and int(plain.step_buf) == 3
    assert not _same(masked.p, _setup(optimizer, kwargs, table_name)[4].p)


def test_all_active_with_misaligned_buffers():
    """Buffers that start 4 bytes off a 16-byte boundary take the
    element-wise form, whatever the table says."""
    kind, h, _s, table, masked = _setup("Adam", {}, "aligned", shift=1)
    assert masked.p.data_ptr() % 16 == 4
    plain = masked.clone()
    for step, g in enumerate(masked.grads, 1):
        plain.step(kind, h, g, step)
        masked.step(kind, h, g, step, _mask([1] * G), table)
    for a, b in zip(masked.buffers(), plain.buffers()):
        assert _same(a, b)


@pytest.mark.parametrize("table_name", list(TABLES))
@pytest.mark.parametrize("optimizer,kwargs", ARMS, ids=ARM_IDS)
def test_masks_freeze_models_and_leave_the_rest_unchanged(optimizer, kwargs,
                                                          table_name):
    kind, h, sizes, table, state = _setup(optimizer, kwargs, table_name)
    state.step(kind, h, state.grads[0], 1)  # non-trivial slots, step 1
    index = [_model_index(sizes, g) for g in range(G)]
    for mask_name, mask in MASKS.items():
        before = state.clone()
        masked = state.clone()
        plain = state.clone()
        grad = state.grads[1].clone()
        frozen = [g for g in range(G) if not mask[g]]
        active = [g for g in range(G) if mask[g]]
        # a NaN in one frozen and in one active model's gradient
        poisoned = set()
        if frozen:
            grad[index[frozen[0]][0]] = float("nan")
            poisoned.add(frozen[0])
        if active:
            grad[index[active[-1]][-1]] = float("nan")
            poisoned.add(active[-1])
        plain.step(kind, h, grad, 2)
        masked.step(kind, h, grad, 2, _mask(mask), table)
        assert int(masked.step_buf) == 2  # the counter is shared
        names = "p s0 s1 s2 lp".split()
        for name, got, was, want in zip(names, masked.buffers(),
                                        before.buffers(), plain.buffers()):
            for g in range(G):
                ref = want if mask[g] else was
                assert _same(got[index[g]], ref[index[g]]), (
                    mask_name, name, g
                )
                if g not in poisoned or not mask[g]:
                    assert torch.isfinite(got[index[g]].float()).all(), (
                        mask_name, name, g
                    )
        if active:
            # the planted NaN did reach its own model's parameters
            assert torch.isnan(masked.p[index[active[-1]][-1]])


@pytest.mark.parametrize("with_mirror", [True, False])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("table_name", list(TABLES))
def test_masked_copy(table_name, shift, with_mirror):
    require_hip()
    sizes = TABLES[table_name]
    offsets, n = _layout(sizes)
    table = ops.segment_table(offsets, sizes, "cuda")
    gen = torch.Generator().manual_seed(21)
    src_h = (torch.rand(n, generator=gen) * 2 - 1) * 100
    # values whose bf16 rounding is not a truncation, and special ones
    src_h[::7] = 1.00390625          # halfway between two bf16 values
    src_h[3::11] = -0.0
    src_h[5::13] = float("inf")
    src_h[1::17] = 1e-40             # fp32 denormal
    index = [_model_index(sizes, g) for g in range(G)]

    def dev(t):
        buf = torch.empty(n + shift, dtype=t.dtype, device="cuda")
        buf[shift:].copy_(t)
        return buf[shift:]

    src = dev(src_h)
    for mask_name, mask in {**MASKS, "all": [1] * G}.items():
        dst = dev(torch.full((n,), -7.0))
        lp = dev(torch.full((n,), -3.0, dtype=torch.bfloat16))
        ops.masked_copy(dst, src, _mask(mask), table,
                        lp if with_mirror else None)
        want_lp = src.to(torch.bfloat16)
        for g in range(G):
            idx = index[g]
            if mask[g]:
                assert _same(dst[idx], src[idx]), (mask_name, g)
            else:
                assert (dst[idx] == -7.0).all(), (mask_name, g)
            if mask[g] and with_mirror:
                assert _same(lp[idx], want_lp[idx]), (mask_name, g)
            else:
                assert (lp[idx] == -3.0).all(), (mask_name, g)
        assert _same(src, dev(src_h))  # the source is only read


def test_bad_table_entries_are_skipped_not_followed():
    """A table entry that does not fit into the buffer is ignored: the
    kernel never forms an address outside [0, n)."""
    require_hip()
    sizes = (8, 16)
    offsets, n = _layout(sizes)
    good = ops.segment_table(offsets, sizes, "cuda")
    bad = ops.segment_table(
        offsets + [n - 8, -4, 0], list(sizes) + [16, 8, n], "cuda"
    )
    src = torch.arange(n, dtype=torch.float32, device="cuda")
    want = torch.zeros(n, device="cuda")
    got = torch.zeros(n, device="cuda")
    ops.masked_copy(want, src, _mask([1] * G), good)
    ops.masked_copy(got, src, _mask([1] * G), bad)
    assert torch.equal(got, want) and torch.equal(got, src)


def test_masked_entry_checks_its_arguments():
    require_hip()
    kind, h, _sizes, table, state = _setup("Adam", {}, "aligned")
    with pytest.raises(ValueError):
        state.step(kind, h, state.grads[0], 1, _mask([1] * G), None)
    with pytest.raises(RuntimeError):
        state.step(kind, h, state.grads[0], 1, _mask([1] * G).float(), table)
    with pytest.raises(RuntimeError):
        ops.masked_copy(state.p, state.grads[0], _mask([1] * G),
                        table.to(torch.int32))
