"""``plan_gru`` (csrc/scan_plan.h, through ``ops.gru_plan``) with the
two-step family, on the host. What planned before plans as before (bytes
of docs/kernels.md, "Fused GRU scan"); what the fused rule refuses for its
H or F range goes two-step when H % 16 == 0, 16 <= H <= 256, F % 8 == 0;
the rest is refused. Backward rows ask for dX unless F = 0. Two-step
LDS: 2 * rows * (round32(K) + 8) bf16, K = H forward, 3H backward.
"""
import pytest

from gordo_amd import ops

pytestmark = pytest.mark.skipif(
    not ops.hip_available(), reason="the planner lives in the HIP extension"
)

G, B, T = 2, 33, 5


def _big(rows, K):
    return 2 * rows * (((K + 31) & ~31) + 8) * 2


# H, F, direction, GORDO_LSTM_ROWS -> family (None: refused), rows, bytes
PLANS = [
    (48, 56, "fwd", None, "gru_fwd", 16, 69888),
    (48, 56, "bwd", None, "gru_bwd", 16, 62080),
    (64, 128, "fwd", 64, "gru_fwd", 32, 149504),
    (64, 128, "bwd", None, "gru_bwd", 16, 130304),
    (128, 56, "fwd", None, "gru_fwd_big", 16, _big(16, 128)),
    (128, 56, "bwd", None, "gru_bwd_big", 16, _big(16, 384)),
    (256, 8, "fwd", 64, "gru_fwd_big", 64, _big(64, 256)),
    # 64 rows of dGh at H = 256 are 198 656 bytes: halved
    (256, 8, "bwd", 64, "gru_bwd_big", 32, _big(32, 768)),
    (64, 136, "fwd", None, "gru_fwd_big", 16, _big(16, 64)),
    (64, 136, "bwd", None, "gru_bwd_big", 16, _big(16, 192)),
    (16, 200, "fwd", None, "gru_fwd_big", 16, _big(16, 16)),
    (16, 200, "bwd", 32, "gru_bwd_big", 32, _big(32, 48)),
    # F = 0, no dX: H alone decides
    (64, 0, "bwd", None, "gru_bwd", 16, 58624),
    (128, 0, "bwd", None, "gru_bwd_big", 16, _big(16, 384)),
] + [(H, F, d, None, None, 0, 0) for H, F in ((72, 56), (40, 136), (272, 8))
     for d in ("fwd", "bwd")]


@pytest.mark.parametrize("H,F,direction,env_rows,family,rows,lds", PLANS)
def test_plan(monkeypatch, H, F, direction, env_rows, family, rows, lds):
    monkeypatch.delenv("GORDO_LSTM_ROWS", raising=False)
    if env_rows:
        monkeypatch.setenv("GORDO_LSTM_ROWS", str(env_rows))
    args = (direction, G, B, T, H, F, direction == "bwd" and F > 0, False)
    plan, why = ops.gru_plan(*args), ops.gru_refusal(*args)
    if family is None:
        assert plan is None and why
        assert H != 72 or ("8 <= H <= 64" in why and "16 <= H <= 256" in why)
        return
    assert why is None and (plan["family"], plan["rows"], plan["lds_bytes"],
            plan["blocks"]) == (family, rows, lds, G * -(-B // rows))
    # the two-step backward never has dX inside
    assert plan["has_dx"] is (None if direction == "fwd"
                              else family == "gru_bwd" and F > 0)

