"""The dispatch arms of the LSTM scan kernels: one row per arm, with the
launch record each must produce. Shared by the planner test
(test_scan_plan.py: what ``ops.scan_plan`` answers, no GPU) and the
device tests (test_lstm_scan_arms_gpu.py, test_lstm_scan_act_gpu.py:
what ``ops.last_scan_launch()`` reports after the kernel ran, and the
fp64 oracle). docs/kernels.md, "Scan dispatch table", lists the arms.
"""
from collections import namedtuple

import pytest

# ---------------------------------------------------------------------------
# the arm tables
# ---------------------------------------------------------------------------
# entry: how the kernel is reached; env: GORDO_LSTM_* switches set for
# the call; shape (G, B, T, H, F) with F = 0 for the xW entry points;
# rows / hf: what the launch record must say.
Arm = namedtuple("Arm", "family entry env shape rows hf")

V2_SMALL = [(2, 70, 12), (1, 1, 1), (2, 16, 2), (1, 100, 20)]
# (H, B, T) triples covering every pair of H in {25, 42, 60},
# B in {1, 33, 100}, T in {1, 2, 20}
HBT = [(25, 1, 1), (42, 33, 2), (60, 100, 20),
       (25, 33, 20), (42, 100, 1), (60, 1, 2),
       (25, 100, 2), (42, 1, 20), (60, 33, 1)]
HF_FUSED = [(8, 8), (48, 56), (64, 128)]
ROW_TILES = [16, 32, 64]


def _v2_arms(direction):
    arms = []
    for hf in (1, 2, 3, 4):
        # the public dispatch takes v2 once G * ceil(B/64) >= 256
        arms.append(Arm(f"{direction}_v2", "public", {},
                        (256, 17, 5, 16 * hf, 0), 64, hf))
        # (2, 70, 12): waves hold 16, 16, 16, 16, 6, 0, 0, 0 live rows
        for G, B, T in V2_SMALL:
            arms.append(Arm(f"{direction}_v2", "v2", {},
                            (G, B, T, 16 * hf, 0), 64, hf))
    arms.append(Arm(f"{direction}_v2", "v2", {}, (1, 30, 144, 32, 0), 64, 2))
    return arms


def _barriered_arms(family, entry, env):
    return [
        Arm(family, entry, dict(env, GORDO_LSTM_ROWS=str(r)),
            (2, B, T, H, 0), r, None)
        for r in ROW_TILES for H, B, T in HBT
    ]


def _big_rows(H, B):
    # 64-row tile when B >= 48 and rows * ((Kp + 8) * 2 + ldg * 2 + H * 4)
    # fits 160 KB; at H = 256 (ldg = 1032) 64 rows need 226 KB
    return 64 if B >= 48 and H < 256 else 32


def _big_arms(direction):
    return [
        Arm(f"{direction}_big", "public", {},
            (1 if H == 256 else 2, B, 6, H, 0), _big_rows(H, B), None)
        for H in (72, 128, 256) for B in (20, 48)
    ]


# row tile the v4 forward's LDS budget leaves: [Wh ; Wx]^T plus 64 rows
# of x/h, gates and c need 174.5 KB of the 160 KB at (H, F) = (64, 128)
def _v4_rows(H, F, rows):
    return 32 if (H, F) == (64, 128) and rows == 64 else rows


# ... and the pipelined backward's (pipe_rows(): the tile plus two ring
# slots per row). With dX: (64, 128) fits only 16 rows (145.5 KB; 32
# rows need 192 KB), (48, 56) fits 32 (109 KB; 64 rows need 177.6 KB,
# 165.6 KB last_only). Without dX: H = 64 fits 32 rows (118 KB; 64 rows
# need 203 KB), H = 48 fits 64 (148.75 KB).
def _pipe_rows(H, F, rows, has_dx):
    if has_dx:
        cap = {(8, 8): 64, (48, 56): 32, (64, 128): 16}[(H, F)]
    else:
        cap = {8: 64, 48: 64, 64: 32}[H]
    return min(rows, cap)


FWD_ARMS = (
    _v2_arms("fwd")
    + _barriered_arms("fwd_v3", "public", {})
    + _barriered_arms("fwd_v1", "public", {"GORDO_LSTM_V1": "1"})
    + _big_arms("fwd")
)

BWD_ARMS = (
    _v2_arms("bwd")
    # H % 8 != 0: the bottom-layer entry keeps the old v3 kernel
    + _barriered_arms("bwd_v3", "public", {})
    + _barriered_arms("bwd_v1", "public", {"GORDO_LSTM_V1": "1"})
    # H % 8 == 0: the same entry takes the pipelined kernel without dX
    + [Arm("bwd_pipe", "v3", {"GORDO_LSTM_ROWS": str(r)}, (2, 33, 6, H, 0),
           _pipe_rows(H, 0, r, False), None)
       for r in ROW_TILES for H, _ in HF_FUSED]
    + _big_arms("bwd")
)

V4_ARMS = [
    Arm("fwd_v4", "fused", {"GORDO_LSTM_ROWS": str(r)}, (2, 33, 6, H, F),
        _v4_rows(H, F, r), None)
    for r in ROW_TILES for H, F in HF_FUSED
]

FUSED_BWD_ARMS = [
    Arm("bwd_pipe", "fused", {"GORDO_LSTM_ROWS": str(r)}, (2, 33, 6, H, F),
        _pipe_rows(H, F, r, True), None)
    for r in ROW_TILES for H, F in HF_FUSED
] + [
    # the v5 kernel's smaller footprint keeps the forced tile everywhere
    Arm("bwd_v5", "fused",
        {"GORDO_LSTM_ROWS": str(r), "GORDO_LSTM_PIPE": "0"},
        (2, 33, 6, H, F), r, None)
    for r in ROW_TILES for H, F in HF_FUSED
]


def _arm_id(a):
    G, B, T, H, F = a.shape
    env = "".join(
        f"-{k.replace('GORDO_LSTM_', '').lower()}{v}"
        for k, v in sorted(a.env.items())
    )
    return f"{a.family}-{a.entry}-G{G}B{B}T{T}H{H}F{F}{env}"


def _params(arms):
    return [pytest.param(a, id=_arm_id(a)) for a in arms]


def _set_env(monkeypatch, env):
    for k in ("GORDO_LSTM_V1", "GORDO_LSTM_ROWS", "GORDO_LSTM_PIPE",
              "GORDO_LSTM_V4"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


SAT_ARMS = [
    Arm("fwd_v1", "public", {"GORDO_LSTM_V1": "1"}, (1, 20, 4, 42, 0), 16,
        None),
    Arm("fwd_v2", "v2", {}, (1, 20, 4, 48, 0), 64, 3),
    Arm("fwd_v3", "public", {}, (1, 20, 4, 42, 0), 16, None),
    Arm("fwd_v4", "fused", {}, (1, 20, 4, 48, 56), 16, None),
    Arm("fwd_big", "public", {}, (1, 20, 4, 128, 0), 32, None),
]
