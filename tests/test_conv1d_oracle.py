"""CPU: the fp64 Conv1D oracles against torch.nn.functional.conv1d on
explicitly padded fp64 inputs and against its autograd; the raw-spec
parser's accepted and refused Conv1D specs; host-only planner rows."""
import pytest
import torch
import torch.nn.functional as F

from conv1d_cases import CASES, IDS, reference
from gordo_amd import ops
from gordo_amd.engine.pack import Conv1DPack, pack_class
from gordo_amd.machine.model.models import _parse_raw_spec
from gordo_amd.ops import reference as ref


def _torch_conv(x, W, b, act, padding, d):
    """Keras Conv1D through F.conv1d, one model at a time, fp64."""
    G, B, T, Cin = x.shape
    k = W.shape[1]
    halo = (k - 1) * d
    left = halo if padding == "causal" else halo // 2
    outs = []
    for g in range(G):
        xp = F.pad(x[g].transpose(1, 2), (left, halo - left))  # [B,Cin,T+halo]
        w = W[g].permute(2, 1, 0)                              # [Cout,Cin,k]
        outs.append(F.conv1d(xp, w, b[g], dilation=d).transpose(1, 2))
    return ref.apply_act(torch.stack(outs), ref.act_code(act))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_oracles_match_torch_conv1d_and_autograd(i):
    (G, B, T, Cin, Cout, k, d, padding, act) = CASES[i][0]
    r = reference(i)
    x, W, b, dZ = (r[n].double() for n in ("x", "W", "b", "dZ"))
    x.requires_grad_(), W.requires_grad_(), b.requires_grad_()
    z = _torch_conv(x, W, b, "linear", padding, d)
    y = ref.apply_act(z, ref.act_code(act))
    tol = dict(rtol=0, atol=1e-12 * max(1, B * T))
    torch.testing.assert_close(r["fwd"][0], y.detach(), **tol)
    dX, dW, db = torch.autograd.grad(z, (x, W, b), dZ)
    torch.testing.assert_close(r["bwd_data"][0], dX, **tol)
    torch.testing.assert_close(r["wgrad"][0][0], dW, **tol)
    torch.testing.assert_close(r["wgrad"][0][1], db, **tol)
    # the CPU lane of the ops (the CPU pack's kernels) says the same
    torch.testing.assert_close(
        ops.conv1d_fwd(x.detach(), W.detach(), b.detach(), act, padding, d),
        y.detach(), **tol)
    torch.testing.assert_close(
        ops.conv1d_bwd_data(dZ, W.detach(), padding, d), dX, **tol)
    got = ops.conv1d_wgrad(x.detach(), dZ, k, padding, d)
    torch.testing.assert_close(got[0], dW, **tol)
    torch.testing.assert_close(got[1], db, **tol)


def _raw(*convs, tail=({"keras.layers.Flatten": {}},
                       {"keras.layers.Dense": {"units": 4}})):
    return {"keras.Sequential": {"layers": [
        {"keras.layers.Conv1D": c} for c in convs] + list(tail)}}


OK = {"filters": 6, "kernel_size": 3, "padding": "same"}


def test_parser_accepts_a_conv_stack():
    spec = _parse_raw_spec(_raw(
        dict(OK, activation="relu", kernel_regularizer={"l2": 0.1}),
        {"filters": 5, "kernel_size": (2,), "dilation_rate": 4,
         "padding": "causal", "bias_regularizer": "l1"}), {}, 4, 4, 12)
    assert spec.model_type == "conv1d" and spec.lookback_window == 12
    assert pack_class(spec) is Conv1DPack and spec.recurrent
    a, b, dense = spec.layers
    assert (a.units, a.kernel_size, a.dilation, a.padding, a.activation,
            a.kernel_l2) == (6, 3, 1, "same", "relu", 0.1)
    assert (b.units, b.kernel_size, b.dilation, b.padding, b.activation,
            b.bias_l1) == (5, 2, 4, "causal", "linear", 0.01)
    assert dense.kind == "dense" and "kernel_size" not in dense.to_dict()
    assert spec.layers[0].to_dict()["kernel_size"] == 3


@pytest.mark.parametrize("spec, fragment", [
    (_raw(dict(OK, padding="valid")), "padding 'valid'"),
    (_raw({"filters": 6, "kernel_size": 3}), "padding 'valid'"),
    (_raw(dict(OK, strides=2)), "strides 2"),
    (_raw(dict(OK, groups=2)), "groups 2"),
    (_raw(dict(OK, use_bias=False)), "use_bias=False"),
    (_raw(dict(OK, data_format="channels_first")), "data_format"),
    (_raw(dict(OK, activity_regularizer={"l1": 0.1})),
     "activity_regularizer"),
    (_raw(dict(OK, recurrent_regularizer="l2")), "recurrent_regularizer"),
    (_raw(dict(OK, activation="elu")), "Conv1D activation 'elu'"),
    (_raw(OK, tail=({"keras.layers.LSTM": {"units": 4}},
                    {"keras.layers.Dense": {"units": 4}})), "mixes Conv1D"),
    (_raw(OK, tail=({"keras.layers.Dense": {"units": 4}},)),
     "Flatten layer is missing"),
    (_raw(OK, tail=({"keras.layers.Flatten": {}},
                    {"keras.layers.Dense": {"units": 8}},
                    {"keras.layers.Dense": {"units": 4}})),
     "more than one Dense"),
])
def test_parser_refuses_by_name(spec, fragment):
    with pytest.raises(ValueError, match=fragment):
        _parse_raw_spec(spec, {}, 4, 4, 12)


@pytest.mark.parametrize("T, rows", [(1, 16), (5, 16), (17, 32), (32, 32), (64, 64),
                                     (70, 16), (96, 32), (144, 16)])
def test_planner_row_tile_by_T(T, rows):
    for entry in ("fwd", "bwd_data"):
        assert ops.conv1d_plan(entry, 2, 3, T, 8, 8, 3, 1)["rows"] == rows
    assert ops.conv1d_plan("wgrad", 2, 3, T, 8, 8, 3, 1)["rows"] == 32


def test_planner_case_table_ring_chunks_and_refusals():
    for (shape, rows, resident, chunks, _what) in CASES:
        G, B, T, Cin, Cout, k, d, padding, _act = shape
        for entry in ("fwd", "bwd_data"):
            p = ops.conv1d_plan(entry, G, B, T, Cin, Cout, k, d, padding)
            assert (p["rows"], p["taps_resident"]) == (rows, resident), shape
            assert p["lds_bytes"] <= 160 * 1024
        p = ops.conv1d_plan("wgrad", G, B, T, Cin, Cout, k, d, padding)
        assert p["chunks"] == chunks and p["lds_bytes"] <= 160 * 1024
    # all taps beside the image: 3 x 128 x 136 x 2 B fits, 8 do not
    assert ops.conv1d_plan("fwd", 1, 1, 16, 128, 128, 3)["taps_resident"]
    assert not ops.conv1d_plan("fwd", 1, 1, 16, 128, 128, 8)["taps_resident"]
    # over budget at 64 rows with a 64-row halo: the tile is halved
    assert ops.conv1d_plan("fwd", 1, 1, 64, 128, 128, 3, 32)["rows"] == 16
    # about two workgroups per CU
    assert ops.conv1d_plan("fwd", 31, 256, 144, 56, 48, 3)["blocks"] == 496
    for args, fragment in [
        ((1, 1, 8, 136, 8, 3, 1, "same"), "8 <= channels <= 128"),
        ((1, 1, 8, 8, 12, 3, 1, "same"), "multiples of 8"),
        ((1, 1, 8, 8, 8, 9, 1, "same"), "kernel_size <= 8"),
        ((1, 1, 8, 8, 8, 3, 33, "same"), "dilation <= 64"),
        ((1, 1, 1 << 17, 8, 8, 3, 1, "same"), "T < 2^17"),
        ((1, 1, 8, 8, 8, 3, 1, "valid"), "'same' or 'causal'"),
    ]:
        for entry in ("fwd", "bwd_data", "wgrad"):
            assert ops.conv1d_plan(entry, *args) is None
            assert fragment in ops.conv1d_refusal(entry, *args)
