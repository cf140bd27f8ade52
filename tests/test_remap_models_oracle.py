"""``reference.remap_models`` (the CPU lane of ``ops.remap_models`` and
the oracle of the GPU test) against plain per-tensor indexing, the host
validation of the model pairs, and the pack compaction policy."""
import numpy as np
import pytest
import torch

from gordo_amd import ops
from gordo_amd.engine.compaction import (
    check_ratio, ratio_from_env, should_compact,
)
from gordo_amd.ops import reference

PER = [8, 64, 1028, 1025, 3, 1]
G_SRC, G_DST = 5, 3
SENTINEL = -7.0


def _layout(per, G):
    offsets, total = [], 0
    for n in per:
        offsets.append(total)
        total += G * n
    return offsets, total


def _tensors(flat, per, G):
    """The S [G, per_s] tensors of a flat buffer, by plain slicing."""
    offsets, _ = _layout(per, G)
    return [flat[o : o + G * n].view(G, n) for o, n in zip(offsets, per)]


def _setup():
    so, sn = _layout(PER, G_SRC)
    do, dn = _layout(PER, G_DST)
    src = torch.randn(sn, generator=torch.Generator().manual_seed(3))
    dst = torch.full((dn,), SENTINEL)
    return (src, ops.segment_table(so, PER), dst, ops.segment_table(do, PER))


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("entry", [reference.remap_models, ops.remap_models])
def test_gather_then_scatter_against_per_tensor_indexing(entry):
    src, stab, dst, dtab = _setup()
    lp = torch.full((dst.numel(),), -3.0, dtype=torch.bfloat16)
    src_before = src.clone()
    # gather: models 4 and 1 of the big buffer become 2 and 0 of the small
    entry(dst, src, [2, 0], [4, 1], dtab, stab, G_DST, G_SRC, dst_lp=lp)
    assert torch.equal(src, src_before)
    for d, l, s in zip(_tensors(dst, PER, G_DST), _tensors(lp, PER, G_DST),
                       _tensors(src, PER, G_SRC)):
        assert torch.equal(_bits(d[2]), _bits(s[4]))
        assert torch.equal(_bits(d[0]), _bits(s[1]))
        assert torch.equal(_bits(l[2]), _bits(s[4].to(torch.bfloat16)))
        assert torch.equal(_bits(l[0]), _bits(s[1].to(torch.bfloat16)))
        # model 1 of the small buffer was not named: sentinel bits
        assert torch.equal(_bits(d[1]), _bits(torch.full_like(d[1], SENTINEL)))
        assert torch.equal(_bits(l[1]), _bits(torch.full_like(l[1], -3.0)))

    # scatter back into a sentinel-filled big buffer
    back = torch.full_like(src, SENTINEL)
    entry(back, dst, [4, 1], [2, 0], stab, dtab, G_SRC, G_DST)
    for b, s in zip(_tensors(back, PER, G_SRC), _tensors(src, PER, G_SRC)):
        for g in range(G_SRC):
            want = s[g] if g in (4, 1) else torch.full_like(s[g], SENTINEL)
            assert torch.equal(_bits(b[g]), _bits(want)), g


@pytest.mark.parametrize("entry", [reference.remap_models, ops.remap_models])
@pytest.mark.parametrize("dst_index,src_index", [
    ([0, 1], [0]),          # unequal lengths
    ([], []),               # empty
    ([G_DST], [0]),         # an index equal to G (dst side)
    ([0], [G_SRC]),         # an index equal to G (src side)
    ([-1], [0]),            # negative
    ([0], [-1]),
    ([1, 1], [0, 2]),       # a dst model twice
])
def test_bad_pairs_raise_and_leave_dst_alone(entry, dst_index, src_index):
    src, stab, dst, dtab = _setup()
    with pytest.raises(ValueError):
        entry(dst, src, dst_index, src_index, dtab, stab, G_DST, G_SRC)
    assert torch.equal(_bits(dst), _bits(torch.full_like(dst, SENTINEL)))


def test_a_src_model_may_be_named_twice():
    src, stab, dst, dtab = _setup()
    ops.remap_models(dst, src, [0, 2], [3, 3], dtab, stab, G_DST, G_SRC)
    for d, s in zip(_tensors(dst, PER, G_DST), _tensors(src, PER, G_SRC)):
        assert torch.equal(d[0], s[3]) and torch.equal(d[2], s[3])


def test_policy_at_the_default_ratio():
    assert not should_compact(5, 3)
    assert should_compact(5, 2)
    assert not should_compact(2, 1)   # a pack of 2 never compacts
    assert should_compact(3, 1)
    assert not should_compact(5, 0)   # nothing left to train
    assert not should_compact(5, 5)


def test_policy_at_ratio_one_compacts_at_every_stop():
    assert should_compact(5, 4, 1.0)
    assert should_compact(2, 1, 1.0)
    assert not should_compact(4, 4, 1.0)


@pytest.mark.parametrize("ratio", [0, 1.5, -0.5, float("nan"), "half"])
def test_bad_ratio_raises(ratio, monkeypatch):
    with pytest.raises(ValueError):
        should_compact(5, 2, ratio)
    with pytest.raises(ValueError):
        check_ratio(ratio)
    monkeypatch.setenv("GORDO_PACK_COMPACT_RATIO", str(ratio))
    with pytest.raises(ValueError):
        ratio_from_env()


def test_ratio_from_env(monkeypatch):
    monkeypatch.delenv("GORDO_PACK_COMPACT", raising=False)
    monkeypatch.delenv("GORDO_PACK_COMPACT_RATIO", raising=False)
    assert ratio_from_env() == 0.5
    monkeypatch.setenv("GORDO_PACK_COMPACT_RATIO", "1.0")
    assert ratio_from_env() == 1.0
    monkeypatch.setenv("GORDO_PACK_COMPACT", "0")
    assert ratio_from_env() is None
