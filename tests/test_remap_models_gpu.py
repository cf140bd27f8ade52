"""``remap_models_kernel`` (masked_ops.hip): whole models between two
flat buffers of different G, bit for bit what ``reference.remap_models``
does on CPU copies, the bf16 mirror included, and not one bit outside
the named models' slices."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops
from gordo_amd.ops import reference

# per-model sizes: vector-width and odd segments, one of exactly one
# unit (1024) and one just past it (1028), and 1025: every base after
# it is odd in one layout or the other
PER = [8, 64, 1028, 1025, 3, 1]
SENTINEL, SENTINEL_LP = -7.0, -3.0


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def _layout(per, G):
    offsets, total = [], 0
    for n in per:
        offsets.append(total)
        total += G * n
    return offsets, total


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _values(n, seed=21):
    """As test_masked_opt_gpu.py draws them for masked_copy: values
    whose bf16 rounding is not a truncation, and special ones."""
    gen = torch.Generator().manual_seed(seed)
    v = (torch.rand(n, generator=gen) * 2 - 1) * 100
    v[::7] = 1.00390625          # halfway between two bf16 values
    v[3::11] = -0.0
    v[5::13] = float("inf")
    v[1::17] = 1e-40             # fp32 denormal
    return v


def _dev(t, shift):
    # shift > 0 moves the buffer off its 16-byte alignment (a buf[1:]
    # view)
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device="cuda")
    buf[shift:].copy_(t)
    return buf[shift:]


def _check(per, G_src, G_dst, dst_index, src_index, shifts=(0, 0, 0),
           mirror=True):
    """Run the op on the GPU and the reference on CPU copies; both
    results must agree bit for bit (sentinels included). Returns the
    GPU (dst, dst_lp) on the host."""
    require_hip()
    so, sn = _layout(per, G_src)
    do, dn = _layout(per, G_dst)
    src_h = _values(sn)
    dst_h = torch.full((dn,), SENTINEL)
    lp_h = torch.full((dn,), SENTINEL_LP, dtype=torch.bfloat16)
    want, want_lp = dst_h.clone(), lp_h.clone()
    reference.remap_models(
        want, src_h, dst_index, src_index, ops.segment_table(do, per),
        ops.segment_table(so, per), G_dst, G_src,
        want_lp if mirror else None,
    )
    dst, src, lp = (_dev(dst_h, shifts[0]), _dev(src_h, shifts[1]),
                    _dev(lp_h, shifts[2]))
    ops.remap_models(
        dst, src, dst_index, src_index, ops.segment_table(do, per, "cuda"),
        ops.segment_table(so, per, "cuda"), G_dst, G_src,
        lp if mirror else None,
    )
    torch.cuda.synchronize()
    got, got_lp = dst.cpu(), lp.cpu()
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(got_lp), _bits(want_lp))
    assert torch.equal(_bits(src.cpu()), _bits(src_h))  # only read
    # the oracle did move something, and did leave something alone
    moved = int((_bits(want) != _bits(dst_h)).sum())
    assert moved > 0
    if len(dst_index) < G_dst:
        assert moved < dn
    return got, got_lp


@pytest.mark.parametrize("mirror", [True, False])
@pytest.mark.parametrize("G_src,G_dst,dst_index,src_index", [
    (5, 3, [2, 0], [4, 1]),            # gather, permuted
    (5, 3, [1, 2, 0], [0, 4, 2]),      # gather, a full small pack
    (3, 5, [4, 1], [2, 0]),            # scatter back
    (3, 5, [3, 0, 2], [1, 2, 0]),
    (5, 3, [1], [3]),                  # a single pair
    (5, 5, [4, 3, 2, 1, 0], [0, 1, 2, 3, 4]),
])
def test_mixed_layout(G_src, G_dst, dst_index, src_index, mirror):
    _check(PER, G_src, G_dst, dst_index, src_index, mirror=mirror)


@pytest.mark.parametrize("per", [
    [8], [5], [1024], [1028],           # S = 1; the unit boundary
    [1024, 1028],
    [1] * 256,                          # S = 256, the table's limit
], ids=["s1-vec", "s1-odd", "s1-unit", "s1-unit+4", "unit-pair", "s256"])
def test_table_shapes(per):
    _check(per, 4, 2, [1, 0], [3, 1])
    _check(per, 2, 4, [3, 1], [1, 0])


@pytest.mark.parametrize("G_src,G_dst", [(4, 3), (3, 4)])
def test_segment_aligned_on_one_side_only(G_src, G_dst):
    """per = [3, 8]: the second tensor starts at 3 * G, a multiple of 4
    for G = 4 and not for G = 3, so it qualifies for 16-byte moves in
    one buffer and not in the other; it moves element-wise, and the
    neighbouring bits stay."""
    n = min(G_src, G_dst)
    _check([3, 8], G_src, G_dst, list(range(n)), list(range(n))[::-1])
    # the same with a 16-byte-movable tensor behind it on both sides
    _check([3, 8, 1, 12], G_src, G_dst, [n - 1], [0])


@pytest.mark.parametrize("shifts", [
    (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 0, 2),
])
def test_misaligned_pointers_give_the_same_bits(shifts):
    aligned = _check(PER, 5, 3, [2, 0], [4, 1])
    shifted = _check(PER, 5, 3, [2, 0], [4, 1], shifts=shifts)
    for a, b in zip(aligned, shifted):
        assert torch.equal(_bits(a), _bits(b))


def test_more_units_than_blocks():
    """64 pairs cap the grid at 64 blocks per model; a model of 71
    units makes every block walk more than one."""
    G = 64
    order = list(range(G))
    _check([70 * 1024 + 4, 5], G, G, order, order[::-1])


@pytest.mark.parametrize("dst_index,src_index", [
    ([0, 1], [0]), ([], []), ([3], [0]), ([0], [5]), ([-1], [0]),
    ([1, 1], [0, 2]),
])
def test_bad_pairs_raise_before_any_launch(dst_index, src_index):
    require_hip()
    so, sn = _layout(PER, 5)
    do, dn = _layout(PER, 3)
    src = _values(sn).cuda()
    dst = torch.full((dn,), SENTINEL, device="cuda")
    with pytest.raises(ValueError):
        ops.remap_models(
            dst, src, dst_index, src_index,
            ops.segment_table(do, PER, "cuda"),
            ops.segment_table(so, PER, "cuda"), 3, 5,
        )
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()
    # the extension's own entry checks them again
    hip = ops.api._require_hip()
    with pytest.raises(RuntimeError):
        hip.remap_models(
            dst, src, dst_index, src_index,
            ops.segment_table(do, PER, "cuda"),
            ops.segment_table(so, PER, "cuda"), 3, 5,
        )
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()


def test_entry_checks_its_tensors():
    require_hip()
    so, sn = _layout(PER, 5)
    do, dn = _layout(PER, 3)
    src = _values(sn).cuda()
    dst = torch.full((dn,), SENTINEL, device="cuda")
    dtab = ops.segment_table(do, PER, "cuda")
    stab = ops.segment_table(so, PER, "cuda")
    with pytest.raises(RuntimeError):   # tables of different S
        ops.remap_models(dst, src, [0], [0], dtab[:, :3].contiguous(), stab,
                         3, 5)
    with pytest.raises(RuntimeError):   # int32 table
        ops.remap_models(dst, src, [0], [0], dtab.to(torch.int32), stab, 3, 5)
    with pytest.raises(RuntimeError):   # a mirror of another size
        ops.remap_models(dst, src, [0], [0], dtab, stab, 3, 5,
                         torch.zeros(dn + 1, dtype=torch.bfloat16,
                                     device="cuda"))
    with pytest.raises(RuntimeError):   # buffer no multiple of its G
        ops.remap_models(dst[:-1], src, [0], [0], dtab, stab, 3, 5)
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()


def test_segments_that_do_not_match_are_skipped():
    """The device-side check of both tables: a tensor whose per-model
    size differs between the tables, or whose entry does not fit its
    buffer, is left out; the others move."""
    require_hip()
    per = [8, 16, 4]
    G_src, G_dst = 4, 2
    so, sn = _layout(per, G_src)
    do, dn = _layout(per, G_dst)
    src_h = _values(sn)
    src = src_h.cuda()
    good_d = ops.segment_table(do, per)
    good_s = ops.segment_table(so, per)
    # tensor 1 claims 12 per model in dst and 16 in src (either way it
    # lies inside both buffers); tensor 2's dst offset leaves the buffer
    bad_d = ops.segment_table([do[0], do[1], dn], [8, 12, 4])
    want = torch.full((dn,), SENTINEL)
    only_first = ops.segment_table(do[:1], per[:1])
    reference.remap_models(want, src_h, [0, 1], [3, 1], only_first,
                           ops.segment_table(so[:1], per[:1]), G_dst, G_src)
    got = torch.full((dn,), SENTINEL, device="cuda")
    ops.remap_models(got, src, [0, 1], [3, 1], bad_d.cuda(), good_s.cuda(),
                     G_dst, G_src)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got.cpu()), _bits(want))
    # and with the good tables everything moves
    full = torch.full((dn,), SENTINEL, device="cuda")
    ops.remap_models(full, src, [0, 1], [3, 1], good_d.cuda(), good_s.cuda(),
                     G_dst, G_src)
    assert not (full == SENTINEL).any()
