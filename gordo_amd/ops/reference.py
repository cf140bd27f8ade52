"""
CPU/fp32 reference implementations of every device op.

These are the numerics oracles: each HIP kernel in ``csrc/`` is tested
against the same-named function here (tests/test_ops_gpu.py), and they
are the execution path on hosts without a GPU (the CPU test lane).
The LSTM scan and threshold-statistics oracles further down compute
in fp64 and are test-only, as are the ``*_ref`` oracles of the grouped
GEMM and pointwise training ops at the end.

Layouts (G = models in the pack, B = rows, In/Out = features):
    X   [G, B, In]
    W   [G, In, Out]
    b   [G, Out]
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

ACT_LINEAR, ACT_TANH, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3

_ACT_NAMES = {
    "linear": ACT_LINEAR,
    None: ACT_LINEAR,
    "tanh": ACT_TANH,
    "relu": ACT_RELU,
    "sigmoid": ACT_SIGMOID,
}


def act_code(name) -> int:
    if isinstance(name, int):
        return name
    try:
        return _ACT_NAMES[name]
    except KeyError:
        raise ValueError(f"Unsupported activation {name!r}") from None


def apply_act(z: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_LINEAR:
        return z
    if act == ACT_TANH:
        return torch.tanh(z)
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    raise ValueError(f"Unknown activation code {act}")


def act_grad_from_output(y: torch.Tensor, act: int) -> torch.Tensor:
    """d act / d z expressed from the activation OUTPUT y (tanh: 1-y²,
    sigmoid: y(1-y), relu: 1[y>0]) — what the fused kernel computes."""
    if act == ACT_LINEAR:
        return torch.ones_like(y)
    if act == ACT_TANH:
        return 1.0 - y * y
    if act == ACT_RELU:
        return (y > 0).to(y.dtype)
    if act == ACT_SIGMOID:
        return y * (1.0 - y)
    raise ValueError(f"Unknown activation code {act}")


def grouped_linear_fwd(
    X: torch.Tensor, W: torch.Tensor, b: torch.Tensor, act: int
) -> torch.Tensor:
    """Y = act(X @ W + b) per group."""
    z = torch.baddbmm(b.unsqueeze(1), X, W)
    return apply_act(z, act)


def act_l1_bwd(
    dA: torch.Tensor, Y: torch.Tensor, act: int, l1: float
) -> torch.Tensor:
    """dZ = (dA + l1*sign(Y)) * act'(z), with act' from output Y.

    The l1 term is the gradient of an L1 activity regularizer on the
    activation output (reference: keras l1(1e-4) activity_regularizer,
    feedforward_autoencoder.py:81)."""
    g = dA if l1 == 0.0 else dA + l1 * torch.sign(Y)
    return g * act_grad_from_output(Y, act)


def grouped_linear_bwd_data(dZ: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """dX = dZ @ W^T per group."""
    return torch.bmm(dZ, W.transpose(1, 2))


def grouped_linear_wgrad(
    X: torch.Tensor, dZ: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    """dW = X^T @ dZ;  db = sum_rows dZ."""
    dW = torch.bmm(X.transpose(1, 2), dZ)
    db = dZ.sum(dim=1)
    return dW, db


def grouped_gemm_acc(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor):
    """C += A @ B per group, in place (the LSTM recurrent-gate GEMM
    accumulating onto the precomputed x-side gates)."""
    C.baddbmm_(A, B)
    return C


def mse_bwd(
    Y: torch.Tensor, T: torch.Tensor, real_n: int = -1
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-model MSE loss and its gradient.

    loss[g] = mean((Y-T)^2) over (B, F); dY = 2 (Y-T) / (B*F).
    ``real_n`` overrides the divisor when the feature dim carries zero
    padding (pad diffs are exactly 0; only the mean's count changes).
    """
    diff = Y - T
    n = Y.shape[1] * Y.shape[2] if real_n <= 0 else real_n
    loss = (diff * diff).sum(dim=(1, 2)) / n
    dY = diff * (2.0 / n)
    return loss, dY


LOSS_MSE, LOSS_MAE, LOSS_HUBER, LOSS_LOGCOSH = 0, 1, 2, 3

_LOSS_CODES = {
    "mse": LOSS_MSE,
    "mae": LOSS_MAE,
    "huber": LOSS_HUBER,
    "logcosh": LOSS_LOGCOSH,
}


def loss_code(name) -> int:
    """Engine loss code from a CANONICAL loss name (the spec's
    ``loss_kind``); Keras aliases are resolved in engine/spec.py."""
    if isinstance(name, int) and name in _LOSS_CODES.values():
        return name
    try:
        return _LOSS_CODES[name]
    except KeyError:
        raise ValueError(f"Unsupported loss {name!r}") from None


def loss_bwd(
    Y: torch.Tensor,
    T: torch.Tensor,
    loss,
    real_f: int,
    delta: float = 1.0,
    want_grad: bool = True,
) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """Per-model loss, its gradient and the Keras ``accuracy`` count.

    Y, T: [G, B, Fp]; columns >= ``real_f`` are zero padding. With
    d = Y - T the per-element losses are mse d², mae |d|, huber
    (0.5 d² inside ``delta``, linear outside), logcosh log(cosh d); the
    mean divides by B*real_f and dY = l'(d) / (B*real_f).

    correct[g] counts rows whose argmax over the first ``real_f``
    columns agrees between Y and T (first maximum wins ties) — Keras
    categorical accuracy — or, for ``real_f == 1``, rows with
    t == (y > 0.5) — Keras binary accuracy."""
    kind = loss_code(loss)
    d = Y - T
    a = d.abs()
    n = Y.shape[1] * int(real_f)
    if kind == LOSS_MSE:
        l, gr = d * d, 2.0 * d
    elif kind == LOSS_MAE:
        l, gr = a, torch.sign(d)
    elif kind == LOSS_HUBER:
        quad = a <= delta
        l = torch.where(quad, 0.5 * d * d, delta * (a - 0.5 * delta))
        gr = torch.where(quad, d, delta * torch.sign(d))
    else:
        l = a + torch.log1p(torch.exp(-2.0 * a)) - math.log(2.0)
        l = torch.where(a == 0, torch.zeros_like(l), l)  # exactly 0 at 0
        gr = torch.tanh(d)
    loss_out = l.sum(dim=(1, 2)) / n
    dY = gr / n if want_grad else None
    y_r, t_r = Y[..., :real_f], T[..., :real_f]
    if real_f == 1:
        hit = t_r[..., 0] == (y_r[..., 0] > 0.5).to(t_r.dtype)
    else:
        hit = torch.argmax(y_r, dim=-1) == torch.argmax(t_r, dim=-1)
    correct = hit.sum(dim=1).to(torch.int32)
    return loss_out, dY, correct


def optimizer_step(
    kind: str,
    p: torch.Tensor,
    g: torch.Tensor,
    s0: Optional[torch.Tensor],
    s1: Optional[torch.Tensor],
    s2: Optional[torch.Tensor],
    hyper: dict,
    step: int,
    p_lp: Optional[torch.Tensor] = None,
    reg: Optional[torch.Tensor] = None,
    table: Optional[torch.Tensor] = None,
    G: Optional[int] = None,
):
    """One in-place optimizer step over a flat fp32 parameter buffer
    (Keras 3 update rules); refreshes the low-precision mirror when
    given. ``kind`` is the spec's canonical optimizer name, ``hyper``
    its complete ``optimizer_params``; s0/s1/s2 are the state slots
    (m / v / v̂ for Adam; momentum for SGD; v + momentum for RMSprop;
    the accumulator for Adagrad; m / u for Adamax). With ``reg`` (the
    float32 [2, S] coefficient table beside the segment ``table`` of a
    buffer of ``G`` models) the step sees ``regularized_grad`` instead
    of ``g``; ``g`` itself is not modified."""
    if reg is not None:
        g = regularized_grad(p, g, table, reg, G)
    lr = float(hyper["learning_rate"])
    if kind == "adam" and not hyper.get("amsgrad"):
        adam_step(p, g, s0, s1, lr, hyper["beta_1"], hyper["beta_2"],
                  hyper["epsilon"], step, p_lp)
        return
    if kind == "sgd":
        mu = float(hyper["momentum"])
        if mu == 0.0:
            p.add_(g, alpha=-lr)
        else:
            s0.mul_(mu).add_(g, alpha=-lr)
            if hyper.get("nesterov"):
                p.add_(s0, alpha=mu).add_(g, alpha=-lr)
            else:
                p.add_(s0)
    elif kind == "rmsprop":
        rho, mu = float(hyper["rho"]), float(hyper["momentum"])
        s0.mul_(rho).addcmul_(g, g, value=1.0 - rho)
        inc = lr * g / (s0 + float(hyper["epsilon"])).sqrt_()
        if mu > 0.0:
            s1.mul_(mu).add_(inc)
            p.sub_(s1)
        else:
            p.sub_(inc)
    elif kind == "adagrad":
        s0.addcmul_(g, g)
        p.sub_(lr * g / (s0 + float(hyper["epsilon"])).sqrt_())
    elif kind == "adam":  # amsgrad
        b1, b2 = float(hyper["beta_1"]), float(hyper["beta_2"])
        s0.mul_(b1).add_(g, alpha=1.0 - b1)
        s1.mul_(b2).addcmul_(g, g, value=1.0 - b2)
        torch.maximum(s2, s1, out=s2)
        alpha = lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
        p.addcdiv_(s0, s2.sqrt().add_(float(hyper["epsilon"])), value=-alpha)
    elif kind == "adamax":
        b1, b2 = float(hyper["beta_1"]), float(hyper["beta_2"])
        s0.mul_(b1).add_(g, alpha=1.0 - b1)
        torch.maximum(s1 * b2, g.abs(), out=s1)
        p.addcdiv_(s0, s1 + float(hyper["epsilon"]),
                   value=-lr / (1.0 - b1 ** step))
    else:
        raise ValueError(f"Unsupported optimizer {kind!r}")
    if p_lp is not None:
        p_lp.copy_(p)


def adam_step(
    p: torch.Tensor,
    g: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    step: int,
    p_lp: Optional[torch.Tensor] = None,
):
    """Fused Adam over a flat fp32 parameter buffer (in-place); also
    refreshes the low-precision (bf16) mirror when given.

    Matches Keras Adam semantics: bias-corrected m̂/v̂,
    update = lr * m̂ / (sqrt(v̂) + eps).
    """
    m.mul_(beta1).add_(g, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = (v / bc2).sqrt_().add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
    if p_lp is not None:
        p_lp.copy_(p)


def segment_table(offsets, sizes, device=None) -> torch.Tensor:
    """The int64 [2, S] segment table of a flat buffer of S tensors:
    tensor s is [G, sizes[s]] and starts at offsets[s], so model g owns
    [offsets[s] + g*sizes[s], offsets[s] + (g+1)*sizes[s])."""
    return torch.tensor(
        [[int(o) for o in offsets], [int(n) for n in sizes]],
        dtype=torch.int64, device=device,
    ).reshape(2, -1)


def _model_slices(t: torch.Tensor, mask: torch.Tensor, table: torch.Tensor):
    """(rows, [G, per_s] view of t) per segment, rows the masked models."""
    rows = torch.nonzero(mask.reshape(-1) != 0).reshape(-1)
    G = mask.numel()
    for off, per in zip(*table.tolist()):
        yield rows, t[off : off + G * per].view(G, per)


def masked_copy(
    dst: torch.Tensor,
    src: torch.Tensor,
    mask: torch.Tensor,
    table: torch.Tensor,
    dst_lp: Optional[torch.Tensor] = None,
):
    """dst <- src for the slices of the models with ``mask[g] != 0``
    (``table``: see ``segment_table``); ``dst_lp``, when given, gets the
    same slices in its own precision. Everything else stays as it is."""
    for (rows, d), (_, s) in zip(
        _model_slices(dst, mask, table), _model_slices(src, mask, table)
    ):
        d[rows] = s[rows]
    if dst_lp is not None:
        for (rows, d), (_, s) in zip(
            _model_slices(dst_lp, mask, table), _model_slices(src, mask, table)
        ):
            d[rows] = s[rows].to(dst_lp.dtype)


def check_model_pairs(dst_index, src_index, G_dst: int, G_src: int):
    """The (dst model, src model) pairs of ``remap_models`` as two int
    lists. Raises ValueError unless they have the same length >= 1,
    every entry lies in [0, G) of its side and ``dst_index`` holds no
    model twice."""
    di = [int(i) for i in dst_index]
    si = [int(i) for i in src_index]
    if len(di) != len(si) or not di:
        raise ValueError(
            "dst_index and src_index must have the same length >= 1, got "
            f"{len(di)} and {len(si)}"
        )
    for name, idx, G in (("dst", di, G_dst), ("src", si, G_src)):
        bad = [i for i in idx if not 0 <= i < int(G)]
        if bad:
            raise ValueError(
                f"{name}_index entries {bad} are outside [0, {int(G)})"
            )
    if len(set(di)) != len(di):
        raise ValueError(f"dst_index holds a model twice: {di}")
    return di, si


def remap_models(
    dst: torch.Tensor,
    src: torch.Tensor,
    dst_index,
    src_index,
    dst_table: torch.Tensor,
    src_table: torch.Tensor,
    G_dst: int,
    G_src: int,
    dst_lp: Optional[torch.Tensor] = None,
):
    """Whole models between two flat buffers of different G: tensor s
    is [G_src, per_s] at ``src_table[0, s]`` in ``src`` and [G_dst,
    per_s] at ``dst_table[0, s]`` in ``dst``. For every pair j the
    slices of model ``src_index[j]`` of ``src`` are written to model
    ``dst_index[j]`` of ``dst`` (and, in its own precision, of
    ``dst_lp``). Everything else stays as it is; a segment whose size
    differs between the tables is skipped."""
    di, si = check_model_pairs(dst_index, src_index, G_dst, G_src)
    G_dst, G_src = int(G_dst), int(G_src)
    di_t = torch.tensor(di, dtype=torch.long, device=dst.device)
    si_t = torch.tensor(si, dtype=torch.long, device=src.device)
    for (doff, dper), (soff, sper) in zip(
        zip(*dst_table.tolist()), zip(*src_table.tolist())
    ):
        if dper != sper or dper <= 0:
            continue
        rows = src[soff : soff + G_src * sper].view(G_src, sper)[si_t]
        dst[doff : doff + G_dst * dper].view(G_dst, dper)[di_t] = rows
        if dst_lp is not None:
            dst_lp[doff : doff + G_dst * dper].view(G_dst, dper)[di_t] = (
                rows.to(dst_lp.dtype)
            )


def reg_table(l1, l2, device=None) -> torch.Tensor:
    """The float32 [2, S] regularizer table that goes with a segment
    table: row 0 the l1, row 1 the l2 coefficient of each tensor."""
    return torch.tensor(
        [[float(a) for a in l1], [float(b) for b in l2]],
        dtype=torch.float32, device=device,
    ).reshape(2, -1)


def _reg_segments(table: torch.Tensor, reg: torch.Tensor, n: int, G: int):
    """(offset, per-model size, l1, l2) of every tensor with a non-zero
    coefficient whose table entry fits into the n-element buffer (the
    kernels skip the others too)."""
    offs, pers = table.tolist()
    l1s, l2s = reg.tolist()
    for off, per, l1, l2 in zip(offs, pers, l1s, l2s):
        if off < 0 or per <= 0 or off + per * G > n:
            continue
        if l1 != 0.0 or l2 != 0.0:
            yield off, per, l1, l2


def regularized_grad(p, g, table, reg, G: int) -> torch.Tensor:
    """What the optimizer sees under weight regularizers: for a tensor
    with coefficients (l1, l2), ``g + (l1 sgn(p) + (2 l2) p)`` with
    ``sgn(±0) = 0``, every product and sum rounded on its own (the
    expression of ``reg_grad`` in masked_ops.hip); ``g`` unchanged for
    the other tensors. A new tensor of ``g``'s dtype."""
    out = g.clone()
    dt = g.dtype
    for off, per, l1, l2 in _reg_segments(table, reg, p.numel(), int(G)):
        sl = slice(off, off + int(G) * per)
        pi = p[sl].to(dt)
        t1 = torch.tensor(l1, dtype=dt) * torch.sign(pi)
        t2 = torch.tensor(2.0 * l2, dtype=dt) * pi
        out[sl] = g[sl] + (t1 + t2)
    return out


def weight_penalty(p, table, reg, G: int) -> torch.Tensor:
    """Per-model ``sum_s (l1_s sum|w_s| + l2_s sum w_s^2)`` of the flat
    buffer ``p``, float32 [G] (Keras adds this to the model's loss).
    CPU form of the HIP ``weight_penalty``: fp32 throughout, torch's
    own summation order."""
    G = int(G)
    out = torch.zeros(G, dtype=torch.float32, device=p.device)
    for off, per, l1, l2 in _reg_segments(table, reg, p.numel(), G):
        w = p[off : off + G * per].view(G, per).to(torch.float32)
        out += (
            torch.tensor(l1, dtype=torch.float32) * w.abs().sum(dim=1)
            + torch.tensor(l2, dtype=torch.float32) * (w * w).sum(dim=1)
        )
    return out


def optimizer_step_masked(
    kind: str,
    p: torch.Tensor,
    g: torch.Tensor,
    s0: Optional[torch.Tensor],
    s1: Optional[torch.Tensor],
    s2: Optional[torch.Tensor],
    hyper: dict,
    step: int,
    p_lp: Optional[torch.Tensor],
    active: torch.Tensor,
    table: torch.Tensor,
    reg: Optional[torch.Tensor] = None,
):
    """``optimizer_step`` for the models with ``active[g] != 0`` only:
    the parameters, state slots and mirror of every other model keep
    their bits, whatever its gradient holds. The step runs over the
    whole buffer, so an active element sees exactly the arithmetic of
    the unmasked step, and the frozen slices are put back afterwards."""
    frozen = (active.reshape(-1) == 0).to(torch.int32)
    bufs = [t for t in (p, s0, s1, s2, p_lp) if t is not None]
    saved = [t.clone() for t in bufs] if bool(frozen.any()) else []
    optimizer_step(kind, p, g, s0, s1, s2, hyper, step, p_lp, reg=reg,
                   table=table, G=active.numel())
    for t, keep in zip(bufs, saved):
        for (rows, d), (_, s) in zip(
            _model_slices(t, frozen, table), _model_slices(keep, frozen, table)
        ):
            d[rows] = s[rows]


def lstm_pointwise_fwd(
    gates: torch.Tensor, c_prev: torch.Tensor, act="tanh"
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """
    LSTM cell pointwise math (Keras gate order i, f, c(g), o).

    gates: [G, B, 4H] pre-activation (x@Wx + h@Wh + b).
    Returns (h, c, gact) where gact = activated gates [G, B, 4H]
    saved for the backward pass. ``act`` is the cell activation φ of
    the candidate gate and of φ(c); i, f, o stay sigmoid.
    """
    act = act_code(act)
    H = gates.shape[-1] // 4
    i = torch.sigmoid(gates[..., 0 * H : 1 * H])
    f = torch.sigmoid(gates[..., 1 * H : 2 * H])
    g = apply_act(gates[..., 2 * H : 3 * H], act)
    o = torch.sigmoid(gates[..., 3 * H : 4 * H])
    c = f * c_prev + i * g
    h = o * apply_act(c, act)
    gact = torch.cat([i, f, g, o], dim=-1)
    return h, c, gact


def lstm_pointwise_bwd(
    dh: torch.Tensor,
    dc_next: torch.Tensor,
    gact: torch.Tensor,
    c: torch.Tensor,
    c_prev: torch.Tensor,
    act="tanh",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    Backward of the pointwise cell math.

    Inputs: dh (grad wrt h_t), dc_next (grad wrt c_t from t+1),
    gact = [i,f,g,o] activated, c = c_t, c_prev = c_{t-1}.
    Returns (dgates_pre [G,B,4H], dc_prev [G,B,H]). Both derivatives
    of the cell activation ``act`` come from stored values: φ'(z_g)
    from g, φ'(c) from φ(c).
    """
    act = act_code(act)
    H = dh.shape[-1]
    i, f, g, o = (
        gact[..., 0 * H : 1 * H],
        gact[..., 1 * H : 2 * H],
        gact[..., 2 * H : 3 * H],
        gact[..., 3 * H : 4 * H],
    )
    phi_c = apply_act(c, act)
    do = dh * phi_c
    dc = dc_next + dh * o * act_grad_from_output(phi_c, act)
    di = dc * g
    df = dc * c_prev
    dg = dc * i
    dc_prev = dc * f
    dgates = torch.cat(
        [
            di * i * (1.0 - i),
            df * f * (1.0 - f),
            dg * act_grad_from_output(g, act),
            do * o * (1.0 - o),
        ],
        dim=-1,
    )
    return dgates, dc_prev


# ---------------------------------------------------------------------------
# High-precision oracle of the fused LSTM sequence scans. Plain torch,
# independent of every other op here. With ``round_points=True`` values
# pass through bf16 exactly where the scan kernels store or feed back
# bf16: h (before it re-enters the recurrence, and in ``hs``), the
# activated gates ``gacts``, dG (before the dG @ Wh^T carry, and in the
# output) and dX. c, dc and the dh carry stay unrounded. Inputs are
# used as passed: callers wanting the kernel's view pass bf16-rounded
# tensors. With ``round_points=False`` the functions are the exact
# (differentiable) recurrence and its analytic gradient. ``act`` is the
# cell activation φ (g = φ(z_g), h = o·φ(c)); the gates stay sigmoid.
# ---------------------------------------------------------------------------


def _bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def _scan_fwd(gate_x, B, T, Wh, b, dtype, round_points, act="tanh"):
    """gate_x(t) -> x-side pre-activation [G,B,4H] of step t."""
    act = act_code(act)
    rnd = _bf16_round if round_points else (lambda t: t)
    Wh = Wh.to(dtype)
    G, H = Wh.shape[0], Wh.shape[1]
    h = torch.zeros(G, B, H, dtype=dtype)
    c = torch.zeros(G, B, H, dtype=dtype)
    hs, cs, gas = [], [], []
    for t in range(T):
        gates = gate_x(t) + torch.bmm(h, Wh)
        if b is not None:
            gates = gates + b.to(dtype).unsqueeze(1)
        i = torch.sigmoid(gates[..., 0 * H:1 * H])
        f = torch.sigmoid(gates[..., 1 * H:2 * H])
        g = apply_act(gates[..., 2 * H:3 * H], act)
        o = torch.sigmoid(gates[..., 3 * H:4 * H])
        c = f * c + i * g
        h = rnd(o * apply_act(c, act))
        hs.append(h)
        cs.append(c)
        gas.append(rnd(torch.cat([i, f, g, o], dim=-1)))
    return torch.stack(hs, 2), torch.stack(cs, 2), torch.stack(gas, 2)


def lstm_seq_fwd_ref(xW, Wh, *, dtype=torch.float64, round_points=True,
                     act="tanh"):
    """Forward scan over precomputed x-side gates xW [G,B,T,4H] with
    Wh [G,H,4H] (gate order i, f, g, o; h_0 = c_0 = 0). Returns
    ``(hs [G,B,T,H], cs [G,B,T,H], gacts [G,B,T,4H])`` in ``dtype``."""
    xW = xW.to(dtype)
    return _scan_fwd(lambda t: xW[:, :, t], xW.shape[1], xW.shape[2], Wh,
                     None, dtype, round_points, act)


def lstm_seq_fwd_fused_ref(x, Wx, Wh, b, *, dtype=torch.float64,
                           round_points=True, act="tanh"):
    """Same scan with the x-side product x_t @ Wx + b formed inside the
    step and added unrounded (x [G,B,T,F], Wx [G,F,4H], b [G,4H])."""
    x, Wx = x.to(dtype), Wx.to(dtype)
    return _scan_fwd(lambda t: torch.bmm(x[:, :, t], Wx), x.shape[1],
                     x.shape[2], Wh, b, dtype, round_points, act)


def lstm_seq_bwd_ref(dSeq, gacts, cs, Wh, last_only, *, Wx=None,
                     dtype=torch.float64, round_points=True, act="tanh"):
    """Reverse (BPTT) scan: pre-activation gate grads dG [G,B,T,4H]
    from upstream grads on the h sequence (dSeq [G,B,T,H], or [G,B,H]
    on h_{T-1} alone when ``last_only``) and the forward's ``gacts`` /
    ``cs``. With ``Wx`` [G,F,4H] also returns dX = dG @ Wx^T."""
    act = act_code(act)
    rnd = _bf16_round if round_points else (lambda t: t)
    dSeq, gacts, cs, Wh = (t.to(dtype) for t in (dSeq, gacts, cs, Wh))
    G, B, T, H4 = gacts.shape
    H = H4 // 4
    WhT = Wh.transpose(1, 2)
    WxT = Wx.to(dtype).transpose(1, 2) if Wx is not None else None
    dh_carry = torch.zeros(G, B, H, dtype=dtype)
    dc = torch.zeros(G, B, H, dtype=dtype)
    dG = [None] * T
    dX = [None] * T
    for t in range(T - 1, -1, -1):
        dh = dh_carry
        if not last_only:
            dh = dh + dSeq[:, :, t]
        elif t == T - 1:
            dh = dh + dSeq
        ga = gacts[:, :, t]
        i, f = ga[..., 0 * H:1 * H], ga[..., 1 * H:2 * H]
        g, o = ga[..., 2 * H:3 * H], ga[..., 3 * H:4 * H]
        c_prev = cs[:, :, t - 1] if t > 0 else torch.zeros_like(dc)
        tc = apply_act(cs[:, :, t], act)
        dc = dc + dh * o * act_grad_from_output(tc, act)
        dg_t = rnd(torch.cat([
            dc * g * i * (1.0 - i),
            dc * c_prev * f * (1.0 - f),
            dc * i * act_grad_from_output(g, act),
            dh * tc * o * (1.0 - o),
        ], dim=-1))
        dc = dc * f
        dG[t] = dg_t
        dh_carry = torch.bmm(dg_t, WhT)
        if WxT is not None:
            dX[t] = rnd(torch.bmm(dg_t, WxT))
    if WxT is None:
        return torch.stack(dG, 2)
    return torch.stack(dG, 2), torch.stack(dX, 2)


# ---------------------------------------------------------------------------
# Threshold statistics (K10 trail_min_max, K11 windowed_quantile, K12
# row_quantile; csrc/thresholds.hip). fp64 oracles written from the
# definitions as plain per-window loops: no pandas rolling, numpy
# quantile routines or scipy filters, so the tests can validate them
# against those (tests/test_threshold_oracle.py). Inputs are [R, N]
# (numpy or torch, any float dtype); outputs are numpy fp64.
# ---------------------------------------------------------------------------
def _as_f64_rows(X):
    import numpy as np

    if isinstance(X, torch.Tensor):
        X = X.detach().cpu().to(torch.float64).numpy()
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be [R, N]")
    return X


def _interp_ref(sorted_valid, q):
    """'linear' quantile of an ascending NaN-free sequence: position
    ``q * (n - 1)`` in double, interpolated between the two
    neighbouring order statistics. Returns ``(value, s_lo, s_hi)``;
    all NaN for an empty sequence."""
    n = len(sorted_valid)
    if n == 0:
        return math.nan, math.nan, math.nan
    pos = float(q) * (n - 1)
    lo = int(math.floor(pos))
    hi = lo + 1 if lo + 1 < n else lo
    frac = pos - lo
    s_lo, s_hi = float(sorted_valid[lo]), float(sorted_valid[hi])
    if s_lo == s_hi:  # also keeps inf - inf out of the expression
        return s_lo, s_lo, s_hi
    return s_lo + (s_hi - s_lo) * frac, s_lo, s_hi


def trail_min_max_ref(X, w: int):
    """K10: per row, the maximum over all full trailing windows of the
    window minimum (``rolling(w).min().max()``). A window holding any
    NaN is excluded; a row with no valid window (or ``N < w``) gives
    NaN."""
    import numpy as np

    X = _as_f64_rows(X)
    R, N = X.shape
    out = np.full(R, np.nan)
    for r in range(R):
        best = None
        for i in range(w - 1, N):
            win = X[r, i - w + 1:i + 1]
            if np.isnan(win).any():
                continue
            m = win.min()
            if best is None or m > best:
                best = m
        if best is not None:
            out[r] = best
    return out


def windowed_quantile_ref(X, w: int, q: float, return_neighbours=False):
    """K11: per row ``rolling(w).quantile(q)`` with ``min_periods = w``
    (any NaN in a window gives NaN), 'linear' interpolation; output
    columns are the windows ending at ``w-1 .. N-1``. With
    ``return_neighbours`` also returns the order statistics ``s_lo``,
    ``s_hi`` each value was interpolated between."""
    import numpy as np

    X = _as_f64_rows(X)
    R, N = X.shape
    if w < 1 or w > N:
        raise ValueError("window longer than series")
    no = N - w + 1
    out = np.full((R, no), np.nan)
    s_lo = np.full((R, no), np.nan)
    s_hi = np.full((R, no), np.nan)
    for r in range(R):
        for i0 in range(no):
            win = X[r, i0:i0 + w]
            if np.isnan(win).any():
                continue
            out[r, i0], s_lo[r, i0], s_hi[r, i0] = _interp_ref(
                np.sort(win), q
            )
    if return_neighbours:
        return out, s_lo, s_hi
    return out


def row_quantile_ref(X, q: float, return_neighbours=False):
    """K12: per row quantile over the non-NaN values, 'linear'
    interpolation; a row without valid values gives NaN."""
    import numpy as np

    X = _as_f64_rows(X)
    R = X.shape[0]
    out = np.full(R, np.nan)
    s_lo = np.full(R, np.nan)
    s_hi = np.full(R, np.nan)
    for r in range(R):
        row = X[r]
        valid = np.sort(row[~np.isnan(row)])
        out[r], s_lo[r], s_hi[r] = _interp_ref(valid, q)
    if return_neighbours:
        return out, s_lo, s_hi
    return out


# ---------------------------------------------------------------------------
# Smoothing (csrc/smoothing.hip: smm, sma, ewma). fp64 oracle written
# from the definitions; no pandas rolling or ewm, so
# tests/test_smoothing_oracle.py can validate it against them. NaN and
# +-inf are missing values in all three methods.
# ---------------------------------------------------------------------------
SMOOTH_METHODS = ("smm", "sma", "ewma")


def _smooth_one(X, w: int, method: str):
    import numpy as np

    R, N = X.shape
    valid = np.isfinite(X)
    out = np.full((R, N), np.nan)
    if method == "ewma":
        # num and den decay by d = 1 - alpha at every position; a valid
        # value adds x and 1; a missing position repeats the last output
        d = 1.0 - 2.0 / (w + 1.0)
        num = np.zeros(R)
        den = np.zeros(R)
        last = np.full(R, np.nan)
        for t in range(N):
            v = valid[:, t]
            num = num * d + np.where(v, X[:, t], 0.0)
            den = den * d + np.where(v, 1.0, 0.0)
            last = np.where(v, num / np.where(v, den, 1.0), last)
            out[:, t] = last
        return out
    no = N - w + 1
    if no <= 0:
        return out  # no full window
    bad = np.zeros((R, no), dtype=np.int64)  # missing values per window
    for k in range(w):
        bad += ~valid[:, k:k + no]
    if method == "sma":
        # each window's own values, added in ascending time order
        acc = np.zeros((R, no))
        clean = np.where(valid, X, 0.0)
        for k in range(w):
            acc = acc + clean[:, k:k + no]
        res = acc / float(w)
    else:
        res = np.empty((R, no))
        for r in range(R):
            for i0 in range(no):
                if bad[r, i0]:
                    res[r, i0] = np.nan
                    continue
                s = np.sort(X[r, i0:i0 + w])
                res[r, i0] = (s[(w - 1) // 2] + s[w // 2]) / 2.0
    out[:, w - 1:] = np.where(bad > 0, np.nan, res)
    return out


def smooth_ref(X, w: int, method: str):
    """``smooth`` oracle: per row of X [R, N] the rolling median (smm,
    ``min_periods = w``), the rolling mean (sma, same) or the span-``w``
    exponentially weighted mean (ewma, ``adjust=True``,
    ``ignore_na=False``) in fp64, full [R, N] output. Returns
    ``(value, value_abs)``: the statistic of x and the same statistic of
    ``|x|``, which the tests scale their bounds by."""
    import numpy as np

    if method not in SMOOTH_METHODS:
        raise ValueError(f"Unknown smoothing method {method!r}")
    w = int(w)
    if w < 1:
        raise ValueError("window must be at least 1")
    X = _as_f64_rows(X)
    return _smooth_one(X, w, method), _smooth_one(np.abs(X), w, method)


# ---------------------------------------------------------------------------
# Grouped GEMM and pointwise training ops: fp64 oracles written from
# the definitions (explicit sums over the contracted index, no bmm), so
# tests/test_gemm_oracle.py can validate them against torch.bmm and
# autograd. Callers pass the kernel's view of the inputs: operands
# already rounded to bf16 (any float dtype holding those values), fp32
# for bias, c, dc and the optimizer state. Every oracle returns
# ``(want, emu)``: the fp64 value and the same computation carried out
# in fp32 on the CPU. ``|emu - want|`` measures what fp32 arithmetic
# alone costs at that shape, which is what the tests scale their
# absolute tolerance from. Test-only, like the scan oracles above.
# ---------------------------------------------------------------------------
def _contract(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """sum_k A[g, m, k] * B[g, k, n], one k at a time."""
    out = torch.zeros(A.shape[0], A.shape[1], B.shape[2], dtype=A.dtype)
    for k in range(A.shape[2]):
        out += A[:, :, k:k + 1] * B[:, k:k + 1, :]
    return out


def _both(fn):
    """(fn in fp64, fn in fp32)."""
    return fn(torch.float64), fn(torch.float32)


def grouped_linear_fwd_ref(X, W, b, act):
    """act(sum_k X[g,m,k] W[g,k,n] + b[g,n])."""
    act = act_code(act)

    def run(dt):
        z = _contract(X.to(dt), W.to(dt)) + b.to(dt).unsqueeze(1)
        return apply_act(z, act)

    return _both(run)


def grouped_linear_bwd_data_ref(dZ, W):
    """dX[g,m,k] = sum_n dZ[g,m,n] W[g,k,n]."""
    return _both(
        lambda dt: _contract(dZ.to(dt), W.to(dt).transpose(1, 2).contiguous())
    )


def grouped_gemm_acc_ref(A, B, C0):
    """C0[g,m,n] + sum_k A[g,m,k] B[g,k,n] (C0 holds bf16 values)."""
    return _both(lambda dt: C0.to(dt) + _contract(A.to(dt), B.to(dt)))


def act_l1_bwd_ref(dA, Y, act, l1):
    """(dA + l1 sign(Y)) act'(Y), act' from the output; sign(±0) = 0
    and relu'(±0) = 0. ``l1`` is used as the fp32 value the kernel
    receives."""
    act = act_code(act)
    l1 = float(torch.tensor(l1, dtype=torch.float32))

    def run(dt):
        y, g = Y.to(dt), dA.to(dt)
        if l1 != 0.0:
            g = g + l1 * torch.sign(y)
        return g * act_grad_from_output(y, act)

    return _both(run)


def mse_bwd_ref(Y, T, real_n: int = -1):
    """loss[g] = sum (Y-T)^2 / n, dY = 2 (Y-T) / n over each model's
    elements; n = ``real_n`` if positive, else the per-model count.
    Returns ``((loss, dY) fp64, (loss, dY) fp32)``. The fp32 loss is a
    plain left-to-right running sum in fp32 (numpy ``add.accumulate``
    keeps the dtype; torch's CPU sums are pairwise or accumulate in
    double), the order-free worst case a reduction tree improves on."""
    import numpy as np

    G = Y.shape[0]
    n = Y[0].numel() if real_n <= 0 else int(real_n)

    def run(dt):
        d = (Y.to(dt) - T.to(dt)).reshape(G, -1)
        inv = torch.tensor(1.0, dtype=dt) / n
        sq = d * d
        if dt == torch.float32:
            total = torch.from_numpy(
                np.add.accumulate(sq.numpy(), axis=1, dtype=np.float32)[:, -1]
                .copy()
            )
        else:
            total = sq.sum(dim=1)
        return total * inv, (2.0 * d * inv).reshape(Y.shape)

    return _both(run)


def _cell_act(z, act):
    """φ(z) with the sigmoid spelled like the gates' (1/(1+exp(-z)))."""
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-z))
    return apply_act(z, act)


def lstm_pointwise_fwd_ref(gates, c_prev, act="tanh"):
    """One LSTM cell step from pre-activations [.., 4H] (order i, f,
    g, o) and c_prev [.., H]: ``((h, c, gact) fp64, (...) fp32)``,
    nothing rounded to bf16. ``act`` is the cell activation."""
    act = act_code(act)
    H = gates.shape[-1] // 4

    def run(dt):
        z, cp = gates.to(dt), c_prev.to(dt)
        i = 1.0 / (1.0 + torch.exp(-z[..., 0 * H:1 * H]))
        f = 1.0 / (1.0 + torch.exp(-z[..., 1 * H:2 * H]))
        g = _cell_act(z[..., 2 * H:3 * H], act)
        o = 1.0 / (1.0 + torch.exp(-z[..., 3 * H:4 * H]))
        c = f * cp + i * g
        return o * _cell_act(c, act), c, torch.cat([i, f, g, o], dim=-1)

    return _both(run)


def lstm_pointwise_bwd_ref(dh, dc_next, gact, c, c_prev, act="tanh"):
    """Gradient of that step with respect to the pre-activations and
    c_prev, from the ACTIVATED gates as given (the kernel reads them
    back as bf16): ``((dgates, dc_prev) fp64, (...) fp32)``."""
    act = act_code(act)
    H = dh.shape[-1]

    def run(dt):
        ga = gact.to(dt)
        i, f = ga[..., 0 * H:1 * H], ga[..., 1 * H:2 * H]
        g, o = ga[..., 2 * H:3 * H], ga[..., 3 * H:4 * H]
        d, cc, cp = dh.to(dt), c.to(dt), c_prev.to(dt)
        tc = _cell_act(cc, act)
        dc = dc_next.to(dt) + d * o * act_grad_from_output(tc, act)
        dgates = torch.cat([
            dc * g * i * (1.0 - i),
            dc * cp * f * (1.0 - f),
            dc * i * act_grad_from_output(g, act),
            d * tc * o * (1.0 - o),
        ], dim=-1)
        return dgates, dc * f

    return _both(run)


def adam_step_ref(p, g, m, v, lr, beta1, beta2, eps, step):
    """One Adam step (Keras: m̂ = m/(1-β1^t), v̂ = v/(1-β2^t),
    p -= lr m̂ / (sqrt(v̂) + eps)) from fp32 p, g, m, v, out of place.
    The hyper-parameters are taken as the fp32 values the kernel
    receives. Returns ``((p, m, v) fp64, (p, m, v) fp32)``."""
    lr, beta1, beta2, eps = (
        float(torch.tensor(x, dtype=torch.float32))
        for x in (lr, beta1, beta2, eps)
    )

    def run(dt):
        b1, b2 = (torch.tensor(x, dtype=dt) for x in (beta1, beta2))
        gg = g.to(dt)
        m1 = b1 * m.to(dt) + (1.0 - b1) * gg
        v1 = b2 * v.to(dt) + (1.0 - b2) * gg * gg
        bc1 = 1.0 - b1 ** int(step)
        bc2 = 1.0 - b2 ** int(step)
        lr_t = torch.tensor(lr, dtype=dt)
        p1 = p.to(dt) - lr_t / bc1 * m1 / (torch.sqrt(v1 / bc2) + eps)
        return p1, m1, v1

    return _both(run)


def reg_step_ref(kind, p, g, s0, s1, s2, hyper, step, table, reg, G):
    """One optimizer step of any kind under weight regularizers, out of
    place: the gradient term ``l1 sgn(p) + 2 l2 p`` (``sgn(±0) = 0``)
    of each tensor's coefficients is added to ``g`` and the Keras rule
    of ``optimizer_step`` follows. ``hyper``'s values and the
    coefficients are taken as the fp32 values the kernel receives.
    Returns ``((p, s0, s1, s2) fp64, (...) fp32)``; a slot the caller
    passes as None comes back as None."""
    h32 = {
        k: (v if isinstance(v, bool)
            else float(torch.tensor(float(v), dtype=torch.float32)))
        for k, v in hyper.items()
    }

    def run(dt):
        pp = p.detach().cpu().to(dt, copy=True)
        gg = g.detach().cpu().to(dt)
        slots = [None if s is None else s.detach().cpu().to(dt, copy=True)
                 for s in (s0, s1, s2)]
        optimizer_step(kind, pp, gg, *slots, h32, int(step), None,
                       reg=reg.cpu(), table=table.cpu(), G=int(G))
        return (pp, *slots)

    return _both(run)


def weight_penalty_ref(p, table, reg, G):
    """Per-model ``sum_s (l1_s sum|w_s| + l2_s sum w_s^2)``, [G]:
    ``(fp64, fp32)``. The fp32 value sums each tensor left to right in
    fp32 (numpy ``add.accumulate``, as ``mse_bwd_ref``): the order-free
    worst case that a reduction tree improves on."""
    import numpy as np

    G = int(G)
    p = p.detach().cpu()
    segs = list(_reg_segments(table.cpu(), reg.cpu(), p.numel(), G))

    def run(dt):
        out = torch.zeros(G, dtype=dt)
        for off, per, l1, l2 in segs:
            w = p[off : off + G * per].view(G, per).to(dt)
            a, q = w.abs(), w * w
            if dt == torch.float32:
                a, q = (
                    torch.from_numpy(
                        np.add.accumulate(t.numpy(), axis=1,
                                          dtype=np.float32)[:, -1].copy()
                    )
                    for t in (a, q)
                )
            else:
                a, q = a.sum(dim=1), q.sum(dim=1)
            out = out + (torch.tensor(l1, dtype=dt) * a
                         + torch.tensor(l2, dtype=dt) * q)
        return out

    return _both(run)
