"""The LSTM scan planner (csrc/scan_plan.h through ``ops.scan_plan``),
on the host: no tensor, no GPU.

* every arm row of scan_cases.py plans to the launch record that the
  device tests assert after the kernel ran;
* the LDS sizes quoted in docs/kernels.md;
* the refusals: a non-tanh cell activation is planned only onto the two
  kernels that take one;
* the routing of the public entries, against a table written out here.
"""
import pytest

from gordo_amd import ops
from scan_cases import (
    BWD_ARMS, FUSED_BWD_ARMS, FWD_ARMS, SAT_ARMS, V4_ARMS, _arm_id, _set_env,
)

pytestmark = pytest.mark.skipif(
    not ops.hip_available(), reason="the planner lives in the HIP extension"
)

FWD_ENTRY = {"public": "fwd", "v2": "fwd_v1", "v3": "fwd_v3",
             "fused": "fwd_fused"}
BWD_ENTRY = {"public": "bwd", "v2": "bwd_v1", "v3": "bwd_bottom",
             "fused": "bwd_fused"}
NON_TANH = ("relu", "sigmoid", "linear")
BWD_ENTRIES = ("bwd", "bwd_bottom", "bwd_fused")


def _record(plan):
    return {k: plan[k] for k in ("family", "rows", "hf", "has_dx",
                                 "last_only")}


@pytest.mark.parametrize("arms", [FWD_ARMS, V4_ARMS, SAT_ARMS],
                         ids=["fwd", "v4", "sat"])
def test_forward_arm_rows(arms, monkeypatch):
    for arm in arms:
        _set_env(monkeypatch, arm.env)
        plan = ops.scan_plan(FWD_ENTRY[arm.entry], *arm.shape)
        assert plan is not None, _arm_id(arm)
        assert _record(plan) == dict(
            family=arm.family, rows=arm.rows, hf=arm.hf, has_dx=None,
            last_only=None), _arm_id(arm)
        assert plan["act"] == "tanh"
        G, B = arm.shape[:2]
        assert plan["blocks"] == G * -(-B // arm.rows)


@pytest.mark.parametrize("last_only", [True, False])
@pytest.mark.parametrize("arms", [BWD_ARMS, FUSED_BWD_ARMS],
                         ids=["bwd", "fused"])
def test_backward_arm_rows(arms, last_only, monkeypatch):
    for arm in arms:
        _set_env(monkeypatch, arm.env)
        plan = ops.scan_plan(BWD_ENTRY[arm.entry], *arm.shape,
                             last_only=last_only)
        assert plan is not None, _arm_id(arm)
        pipe = arm.family == "bwd_pipe"
        assert _record(plan) == dict(
            family=arm.family, rows=arm.rows, hf=arm.hf,
            has_dx=(arm.entry == "fused") if pipe else None,
            last_only=last_only if pipe else None), _arm_id(arm)


def test_lds_bytes(monkeypatch):
    _set_env(monkeypatch, {})
    shape = (2, 33, 6, 48, 56)
    for act, want in (("tanh", 66448), ("relu", 72848)):
        plan = ops.scan_plan("fwd_fused", *shape, act=act)
        assert (plan["rows"], plan["lds_bytes"]) == (16, want)
    for last_only, want in ((True, 73600), (False, 76672)):
        plan = ops.scan_plan("bwd_fused", *shape, last_only=last_only)
        assert (plan["family"], plan["rows"]) == ("bwd_pipe", 16)
        assert plan["lds_bytes"] == want
    # 64 rows asked for, halved until the fp32 gate tile fits 160 KB
    _set_env(monkeypatch, {"GORDO_LSTM_ROWS": "64"})
    plan = ops.scan_plan("fwd_fused", 2, 33, 6, 64, 128, act="relu")
    assert (plan["rows"], plan["lds_bytes"]) == (32, 157712)
    assert plan["act"] == "relu"


@pytest.mark.parametrize("act", NON_TANH)
def test_non_tanh_refusals(act, monkeypatch):
    _set_env(monkeypatch, {})
    ok = (2, 3, 2, 8, 8)
    assert ops.scan_plan("fwd_fused", *ok, act=act)["family"] == "fwd_v4"
    for entry in BWD_ENTRIES:
        plan = ops.scan_plan(entry, *ok, act=act)
        assert (plan["family"], plan["act"]) == ("bwd_pipe", act)
    assert ops.lstm_act_scan_available(8, 8)
    assert ops.lstm_layer_mode(2, 3, 8, 8, act) == "fused"
    # the xW forward entries and the forced v2 / v1 backward take none
    for entry in ("fwd", "fwd_v1", "fwd_v3", "bwd_v1"):
        assert ops.scan_plan(entry, *ok, act=act) is None
    for H, F in ((72, 8), (25, 8), (8, 136)):
        shape = (2, 3, 2, H, F)
        assert ops.scan_plan("fwd_fused", *shape, act=act) is None
        assert ops.scan_plan("bwd_fused", *shape, act=act) is None
        assert ops.scan_refusal("bwd_fused", *shape, act=act)
        if F == 8:  # the entries without Wx see only H
            assert ops.scan_plan("bwd", *shape, act=act) is None
            assert ops.scan_plan("bwd_bottom", *shape, act=act) is None
        assert not ops.lstm_act_scan_available(H, F)
        assert ops.lstm_layer_mode(2, 3, H, F, act) == "per_step"
    monkeypatch.setenv("GORDO_LSTM_PIPE", "0")
    for entry in BWD_ENTRIES:
        assert ops.scan_plan(entry, *ok, act=act) is None
    assert ops.scan_plan("fwd_fused", *ok, act=act)["family"] == "fwd_v4"
    assert not ops.lstm_act_scan_available(8, 8)
    assert ops.lstm_layer_mode(2, 3, 8, 8, act) == "per_step"
    _set_env(monkeypatch, {"GORDO_LSTM_V4": "0"})
    # the kernels stay reachable; the engine does not ask for them
    assert ops.scan_plan("fwd_fused", *ok, act=act)["family"] == "fwd_v4"
    assert not ops.lstm_act_scan_available(8, 8)
    assert ops.lstm_layer_mode(2, 3, 8, 8, act) == "per_step"
    # only the exact strings switch
    _set_env(monkeypatch, {"GORDO_LSTM_V4": "00", "GORDO_LSTM_PIPE": "no"})
    assert ops.lstm_act_scan_available(8, 8)


def test_pipe_store_offset_limit(monkeypatch):
    """T = 2^17 is past the pipelined kernel's 32-bit store offsets:
    tanh falls to v5 / v3, another activation is refused."""
    _set_env(monkeypatch, {})
    for T, fused, bottom in ((2 ** 17 - 1, "bwd_pipe", "bwd_pipe"),
                             (2 ** 17, "bwd_v5", "bwd_v3")):
        shape = (1, 1, T, 8, 8)
        assert ops.scan_plan("bwd_fused", *shape)["family"] == fused
        assert ops.scan_plan("bwd_bottom", *shape)["family"] == bottom
        assert ops.scan_plan("bwd", *shape)["family"] == bottom
        for entry in BWD_ENTRIES:
            plan = ops.scan_plan(entry, *shape, act="relu")
            assert (plan is not None) == (fused == "bwd_pipe")


def test_tanh_geometry_refusals(monkeypatch):
    _set_env(monkeypatch, {})
    assert ops.scan_plan("fwd_fused", 2, 3, 2, 25, 8) is None
    assert ops.scan_plan("fwd_fused", 2, 3, 2, 8, 136) is None
    assert ops.scan_plan("bwd_fused", 2, 3, 2, 72, 8) is None
    assert ops.scan_plan("bwd_fused", 2, 3, 2, 8, 136) is None
    assert ops.scan_plan("bwd_fused", 2, 3, 2, 25, 7)["family"] == "bwd_v5"
    for H, served in ((64, True), (72, True), (76, False), (256, True),
                      (264, False)):
        assert (ops.scan_plan("fwd", 2, 3, 2, H) is not None) == served
        assert (ops.scan_plan("bwd", 2, 3, 2, H) is not None) == served
        assert ops.lstm_seq_available(H) == served
    assert ops.lstm_v4_available(64, 128)
    assert not ops.lstm_v4_available(64, 136)
    assert not ops.lstm_v4_available(60, 8)
    with pytest.raises(RuntimeError):
        ops.scan_plan("sideways", 1, 1, 1, 8)


# public entries: family by H, by whether the v2 grid G * ceil(B/64)
# reaches 256 workgroups, and by GORDO_LSTM_V1. (G, B) pairs with
# G * ceil(B/64) = 255 and 256:
UNDER, FILLS = [(255, 17), (51, 320)], [(256, 17), (64, 193)]
#        H    V1 unset: under, fills      V1=1: under, fills
ROUTES_FWD = {
    16:  (("fwd_v3", "fwd_v2"), ("fwd_v2", "fwd_v2")),
    25:  (("fwd_v3", "fwd_v3"), ("fwd_v1", "fwd_v1")),
    48:  (("fwd_v3", "fwd_v2"), ("fwd_v2", "fwd_v2")),
    64:  (("fwd_v3", "fwd_v2"), ("fwd_v2", "fwd_v2")),
    72:  (("fwd_big", "fwd_big"), ("fwd_big", "fwd_big")),
    256: (("fwd_big", "fwd_big"), ("fwd_big", "fwd_big")),
}
# the bottom-layer entry stands where v3 does forward: the pipelined
# kernel when H % 8 == 0, else v3
ROUTES_BWD = {
    16:  (("bwd_pipe", "bwd_v2"), ("bwd_v2", "bwd_v2")),
    25:  (("bwd_v3", "bwd_v3"), ("bwd_v1", "bwd_v1")),
    48:  (("bwd_pipe", "bwd_v2"), ("bwd_v2", "bwd_v2")),
    64:  (("bwd_pipe", "bwd_v2"), ("bwd_v2", "bwd_v2")),
    72:  (("bwd_big", "bwd_big"), ("bwd_big", "bwd_big")),
    256: (("bwd_big", "bwd_big"), ("bwd_big", "bwd_big")),
}


@pytest.mark.parametrize("entry,routes", [("fwd", ROUTES_FWD),
                                          ("bwd", ROUTES_BWD)])
def test_public_routing(entry, routes, monkeypatch):
    for v1, env in enumerate(({}, {"GORDO_LSTM_V1": "1"})):
        _set_env(monkeypatch, env)
        for H, by_v1 in routes.items():
            for fills, grids in enumerate((UNDER, FILLS)):
                for G, B in grids:
                    plan = ops.scan_plan(entry, G, B, 5, H)
                    assert plan["family"] == by_v1[v1][fills], (H, G, B, env)
                    if plan["family"].endswith("v2"):
                        assert (plan["rows"], plan["hf"]) == (64, H // 16)
    # "1" alone switches v1 on
    _set_env(monkeypatch, {"GORDO_LSTM_V1": "true"})
    assert ops.scan_plan(entry, 2, 17, 5, 25)["family"] == entry + "_v3"


def test_engine_layer_modes(monkeypatch):
    _set_env(monkeypatch, {})
    assert ops.lstm_layer_mode(4, 64, 48, 56) == "fused"
    assert ops.lstm_layer_mode(4, 64, 42, 56) == "two_step"
    assert ops.lstm_layer_mode(4, 64, 48, 136) == "two_step"
    assert ops.lstm_layer_mode(4, 64, 300, 8) == "per_step"
    # big-H: only once G * ceil(B/32) reaches 256
    assert ops.lstm_layer_mode(255, 32, 128, 64) == "per_step"
    assert ops.lstm_layer_mode(256, 32, 128, 64) == "two_step"
    assert ops.lstm_layer_mode(128, 33, 128, 64) == "two_step"
    _set_env(monkeypatch, {"GORDO_LSTM_V4": "0"})
    assert ops.lstm_layer_mode(4, 64, 48, 56) == "two_step"
