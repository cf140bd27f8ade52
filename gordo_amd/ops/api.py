"""
Device-op dispatch.

On GPU (ROCm/MI355X) tensors every op runs in the in-tree HIP extension
(``gordo_amd.ops._gordo_hip``, compiled for gfx950 from ``csrc/``); if
the extension is missing on a CUDA-capable host the call FAILS loudly —
there is deliberately no silent eager fallback on GPU. On CPU tensors
the fp32 reference implementations run (the test oracle / CPU lane).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import reference as ref
from .reference import (  # noqa — ACT_* re-exported via gordo_amd.ops
    ACT_LINEAR,
    ACT_TANH,
    ACT_RELU,
    ACT_SIGMOID,
    act_code,
)

_hip = None
_hip_err: Optional[str] = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    try:
        from . import _gordo_hip  # built in-tree by setup.py / __graft_entry__.build()

        _hip = _gordo_hip
    except ImportError as e:
        _hip_err = str(e)
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _require_hip():
    mod = _load_hip()
    if mod is None:
        raise RuntimeError(
            "gordo_amd HIP extension (_gordo_hip) is not built but a GPU "
            f"tensor was passed. Build it with `python setup.py build_ext "
            f"--inplace` (PYTORCH_ROCM_ARCH=gfx950). Import error: {_hip_err}"
        )
    return mod


def _on_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def grouped_linear_fwd(X, W, b, act) -> torch.Tensor:
    act = act_code(act)
    if _on_gpu(X):
        return _require_hip().grouped_linear_fwd(X, W, b, act)
    return ref.grouped_linear_fwd(X, W, b, act)


def act_l1_bwd(dA, Y, act, l1: float) -> torch.Tensor:
    act = act_code(act)
    if _on_gpu(dA):
        return _require_hip().act_l1_bwd(dA, Y, act, float(l1))
    return ref.act_l1_bwd(dA, Y, act, l1)


def grouped_linear_bwd_data(dZ, W) -> torch.Tensor:
    if _on_gpu(dZ):
        return _require_hip().grouped_linear_bwd_data(dZ, W)
    return ref.grouped_linear_bwd_data(dZ, W)


def grouped_linear_wgrad(X, dZ) -> Tuple[torch.Tensor, torch.Tensor]:
    if _on_gpu(X):
        return _require_hip().grouped_linear_wgrad(X, dZ)
    return ref.grouped_linear_wgrad(X, dZ)


def grouped_linear_wgrad_hprev(hs, dZ, T: int):
    """dWh = h_prev^T @ dG over flattened (b, t) rows, where
    h_prev(b, t) = hs[b, t-1] and zero at t == 0 — the in-kernel
    shifted addressing removes the h_prev_all concat from BPTT
    (a full [G,B,T,H] copy per layer per batch)."""
    if _on_gpu(hs):
        return _require_hip().grouped_linear_wgrad_hprev(hs, dZ, int(T))
    G, B, T_, H = hs.shape
    h_prev = torch.cat(
        [torch.zeros_like(hs[:, :, :1]), hs[:, :, :-1]], dim=2
    ).reshape(G, B * T_, H)
    return ref.grouped_linear_wgrad(h_prev, dZ)


def window_gather(X, idx, T: int):
    """K7 sliding-window featurizer: gather [G,B,T,F] lookback windows
    from the resident series [G,N,F] (device analog of
    create_keras_timeseriesgenerator, reference models.py:713-793)."""
    if _on_gpu(X):
        return _require_hip().window_gather(X, idx, int(T))
    G, N, F = X.shape
    B = idx.shape[1]
    rows = idx.unsqueeze(-1).to(torch.long) + torch.arange(T)
    return X.gather(
        1, rows.reshape(G, B * T, 1).expand(G, B * T, F)
    ).view(G, B, T, F)


def grouped_wgrad_xh(seq, hs, dZ, T: int):
    """Combined recurrent weight-grad: (dWx, dWh, db) in one kernel
    pass — dZ is staged once for both GEMMs (it is half of each
    separate call's global traffic)."""
    if _on_gpu(seq):
        out = _require_hip().grouped_wgrad_xh(seq, hs, dZ, int(T))
        return out[0], out[1], out[2]
    dWx, db = ref.grouped_linear_wgrad(seq, dZ)
    dWh, _ = grouped_linear_wgrad_hprev(hs, dZ, T)
    return dWx, dWh, db


def last_wgrad_launch() -> dict:
    """Which weight-grad kernel this thread's last ``grouped_wgrad_xh``
    / ``grouped_linear_wgrad`` / ``grouped_linear_wgrad_hprev`` call
    launched: ``family`` ("wgrad_pipe": the whole-tile kernel with
    16-byte loads and transposed LDS reads; "wgrad_tile": the 64x64
    tile kernel), ``chunks`` (M-chunks, i.e. ``gridDim.y``; more than
    one means fp32 atomics into dW) and ``mstep`` (rows per step).
    Host-side record; ``family`` is "" before any launch.
    ``GORDO_WGRAD_PIPE=0`` forces "wgrad_tile"; ``GORDO_WGRAD_CHUNK``
    forces the chunk length in rows."""
    family, chunks, mstep = _require_hip().last_wgrad_launch()
    return {"family": family, "chunks": chunks, "mstep": mstep}


def grouped_gemm_acc(A, B, C):
    if _on_gpu(A):
        return _require_hip().grouped_gemm_acc(A, B, C)
    return ref.grouped_gemm_acc(A, B, C)


def mse_bwd(Y, T, real_n: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-model MSE loss + grad. ``real_n``: divisor for the mean
    when the feature dim carries zero padding (pad diffs are exactly 0,
    so only the normalization needs the real count)."""
    if _on_gpu(Y):
        return _require_hip().mse_bwd(Y, T, int(real_n))
    return ref.mse_bwd(Y, T, real_n)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, p_lp=None,
              step_buf=None):
    if _on_gpu(p):
        if step_buf is None:
            raise ValueError("GPU adam_step needs a device step_buf")
        return _require_hip().adam_step(
            p, g, m, v, float(lr), float(beta1), float(beta2), float(eps),
            int(step), p_lp, step_buf,
        )
    return ref.adam_step(p, g, m, v, lr, beta1, beta2, eps, step, p_lp)


def loss_bwd(Y, T, loss, real_f: int, delta: float = 1.0,
             want_grad: bool = True):
    """Per-model loss + grad + accuracy count in one pass over (Y, T):
    ``(loss[G] f32, dY | None, correct[G] int32)``. ``loss`` is a
    canonical name (mse/mae/huber/logcosh); ``real_f`` the logical
    feature width when the last dim carries zero padding."""
    kind = ref.loss_code(loss)
    if _on_gpu(Y):
        out = _require_hip().loss_bwd(
            Y, T, kind, int(real_f), float(delta), bool(want_grad)
        )
        return out[0], out[1], out[2]
    return ref.loss_bwd(Y, T, kind, int(real_f), float(delta), want_grad)


# optimizer codes of train_ops.hip (plain Adam keeps adam_kernel; it is
# code 0 of the masked entry in masked_ops.hip)
_OPT_SGD, _OPT_RMSPROP, _OPT_ADAGRAD, _OPT_ADAM_AMSGRAD, _OPT_ADAMAX = (
    1, 2, 3, 4, 5
)
_OPT_ADAM = 0


def segment_table(offsets, sizes, device=None):
    """int64 [2, S] segment table of a flat [S tensors of [G, size_s]]
    buffer (row 0 offsets, row 1 per-model sizes) on ``device``: what
    the masked ops take as ``segments`` / ``table``."""
    return ref.segment_table(offsets, sizes, device)


def masked_copy(dst, src, mask, table, dst_lp=None):
    """Copy the slices of the models with ``mask[g] != 0`` from the
    flat fp32 ``src`` to ``dst`` (and, rounded, into the bf16 mirror
    ``dst_lp``); every other element of ``dst`` / ``dst_lp`` is left
    untouched. ``mask`` is an int32 [G] tensor, ``table`` a
    ``segment_table``, both on the buffers' device."""
    if _on_gpu(dst):
        return _require_hip().masked_copy(dst, src, mask, table, dst_lp)
    return ref.masked_copy(dst, src, mask, table, dst_lp)


def remap_models(dst, src, dst_index, src_index, dst_table, src_table,
                 G_dst, G_src, dst_lp=None):
    """Move whole models between two flat fp32 buffers of different G
    (pack compaction): for every pair j, the slices of model
    ``src_index[j]`` of ``src`` ([G_src, per_s] tensors at
    ``src_table``'s offsets) are written to model ``dst_index[j]`` of
    ``dst`` ([G_dst, per_s] at ``dst_table``'s) and, rounded as
    ``masked_copy`` rounds, into the bf16 mirror ``dst_lp``; every
    other element of ``dst`` / ``dst_lp`` keeps its bits. The index
    sequences are host ints and are checked before anything is
    launched (ValueError): equal length >= 1, every entry inside its
    side's G, no model twice in ``dst_index``."""
    di, si = ref.check_model_pairs(dst_index, src_index, G_dst, G_src)
    if _on_gpu(dst):
        return _require_hip().remap_models(
            dst, src, di, si, dst_table, src_table, int(G_dst), int(G_src),
            dst_lp,
        )
    return ref.remap_models(
        dst, src, di, si, dst_table, src_table, G_dst, G_src, dst_lp
    )


def reg_table(l1, l2, device=None):
    """float32 [2, S] regularizer table beside a ``segment_table``: row
    0 the l1 and row 1 the l2 coefficient of each of the S tensors."""
    return ref.reg_table(l1, l2, device)


def weight_penalty(p, table, reg, G):
    """Per-model weight penalty of the flat fp32 buffer ``p``:
    ``sum_s (l1_s sum|w_s| + l2_s sum w_s^2)`` over the tensors of
    ``table`` with the coefficients of ``reg`` (``reg_table``), float32
    [G]. Reads ``p`` only. On GPU a model's result bits depend on that
    model's values alone: not on G, on its place in the pack, on the
    alignment of its slices or on the launch (no atomics; see
    docs/kernels.md, "Weight regularizers")."""
    if _on_gpu(p):
        return _require_hip().weight_penalty(p, table, reg, int(G))
    return ref.weight_penalty(p, table, reg, int(G))


def last_optimizer_launch() -> dict:
    """Which optimizer kernel this thread's last GPU ``optimizer_step``
    / ``adam_step`` launched: ``family`` ("adam": adam_kernel, "opt":
    opt_kernel<KIND>, "masked": the segment-aware opt_masked_kernel)
    and ``reg`` (the weight regularizers' gradient term was fused in).
    Host-side record; ``family`` is "" before any launch."""
    family, reg = _require_hip().last_optimizer_launch()
    return {"family": family, "reg": bool(reg)}


def optimizer_step(kind, p, g, s0, s1, s2, hyper, step, p_lp=None,
                   step_buf=None, active=None, segments=None, reg=None,
                   G=None):
    """One fused optimizer step over the flat fp32 master buffer (+
    bf16 mirror refresh). ``kind``/``hyper`` are the spec's canonical
    optimizer name and complete ``optimizer_params``. On GPU the step
    counter is read from the device ``step_buf`` (capturable).

    With ``active`` (int32 [G]) and ``segments`` (``segment_table``)
    the step takes the masked entry: a model with ``active[g] == 0`` is
    neither read nor written, an active one gets exactly the unmasked
    arithmetic. Without ``active`` the unmasked kernels run.

    With ``reg`` (``reg_table``, beside ``segments``) the optimizer
    sees ``g + (l1 sgn(p) + 2 l2 p)`` for every tensor with a non-zero
    coefficient (``sgn(±0) = 0``); ``g`` is not modified. The step is
    then the segment-aware one with or without ``active``; without it
    ``G`` (the number of models) must be given."""
    if (active is not None or reg is not None) and segments is None:
        raise ValueError(
            "a masked or regularized optimizer_step needs the segment table"
        )
    if reg is not None and active is None and G is None:
        raise ValueError("a regularized optimizer_step needs active or G")
    if reg is not None:
        G = int(active.numel() if active is not None else G)
    if not _on_gpu(p):
        if active is not None:
            return ref.optimizer_step_masked(
                kind, p, g, s0, s1, s2, hyper, step, p_lp, active, segments,
                reg,
            )
        return ref.optimizer_step(kind, p, g, s0, s1, s2, hyper, step, p_lp,
                                  reg=reg, table=segments, G=G)
    if step_buf is None:
        raise ValueError("GPU optimizer_step needs a device step_buf")
    h = hyper
    lr = float(h["learning_rate"])

    def masked(code, slots, vals, flag):
        ext = _require_hip()
        vals = [float(v) for v in vals]
        if reg is not None:
            return ext.optimizer_step_reg(
                code, p, g, *slots, vals, flag, p_lp, step_buf, active,
                segments, reg, G,
            )
        return ext.optimizer_step_masked(
            code, p, g, *slots, vals, flag, p_lp, step_buf, active, segments,
        )

    segment_aware = active is not None or reg is not None
    if kind == "adam" and not h.get("amsgrad"):
        if segment_aware:
            return masked(
                _OPT_ADAM, (s0, s1, None),
                [lr, h["beta_1"], h["beta_2"], h["epsilon"]], False,
            )
        return _require_hip().adam_step(
            p, g, s0, s1, lr, float(h["beta_1"]), float(h["beta_2"]),
            float(h["epsilon"]), int(step), p_lp, step_buf,
        )
    flag = False
    if kind == "sgd":
        code, vals = _OPT_SGD, [lr, h["momentum"], 0.0, 0.0]
        flag = bool(h.get("nesterov"))
    elif kind == "rmsprop":
        code = _OPT_RMSPROP
        vals = [lr, h["rho"], h["momentum"], h["epsilon"]]
    elif kind == "adagrad":
        code, vals = _OPT_ADAGRAD, [lr, h["epsilon"], 0.0, 0.0]
    elif kind == "adam":
        code = _OPT_ADAM_AMSGRAD
        vals = [lr, h["beta_1"], h["beta_2"], h["epsilon"]]
    elif kind == "adamax":
        code = _OPT_ADAMAX
        vals = [lr, h["beta_1"], h["beta_2"], h["epsilon"]]
    else:
        raise ValueError(f"Unsupported optimizer {kind!r}")
    if segment_aware:
        return masked(code, (s0, s1, s2), vals, flag)
    return _require_hip().optimizer_step(
        code, p, g, s0, s1, s2, [float(v) for v in vals], flag, p_lp,
        step_buf,
    )


# ---- LSTM sequence scans: which kernel serves a call, at which row
# tile, is decided by the extension's host-only planner
# (csrc/scan_plan.h), which also reads the GORDO_LSTM_* switches

def _record(family, rows, hf, has_dx, last_only) -> dict:
    return {
        "family": family,
        "rows": rows,
        "hf": hf if hf > 0 else None,
        "has_dx": None if has_dx < 0 else bool(has_dx),
        "last_only": None if last_only < 0 else bool(last_only),
    }


def _plan(entry, G, B, T, H, F, last_only, act):
    *record, act, lds, blocks, err = _require_hip().scan_plan(
        entry, G, B, T, H, F, bool(last_only), act_code(act))
    if err:
        return None, err
    return dict(_record(*record), act=act, lds_bytes=lds, blocks=blocks), None


def scan_plan(entry, G, B, T, H, F=0, last_only=False, act="tanh"):
    """What a scan call would launch, without touching the GPU: the
    fields of ``last_scan_launch`` plus ``act``, ``lds_bytes`` and
    ``blocks``; ``None`` where the planner refuses (``scan_refusal``
    has the reason). ``entry``: fwd, fwd_v1, fwd_v3, fwd_fused, bwd,
    bwd_v1, bwd_bottom, bwd_fused, as the wrappers below name them."""
    return _plan(entry, G, B, T, H, F, last_only, act)[0]


def scan_refusal(entry, G, B, T, H, F=0, last_only=False, act="tanh"):
    """The planner's message where ``scan_plan`` is None, else None."""
    return _plan(entry, G, B, T, H, F, last_only, act)[1]


def lstm_layer_mode(G: int, B: int, H: int, F: int, act="tanh") -> str:
    """How the engine runs one LSTM layer: "fused" (x-GEMM inside the
    forward scan, dX inside the backward one), "two_step" (x-GEMM,
    then the xW scans) or "per_step" (always, without the extension)."""
    if not hip_available():
        return "per_step"
    return _hip.scan_layer_mode(G, B, H, F, act_code(act))


def lstm_seq_available(H: int) -> bool:
    """Fused sequence-scan coverage: the LDS-resident kernels serve
    H <= 64; the big-H kernels (Wh streamed from L2, 64-column tile
    loop) serve 64 < H <= 256 when H % 8 == 0 — which covers the
    reference's default LSTM dims (256, 128, 64), reference
    gordo/machine/model/factories/lstm_autoencoder.py:112."""
    return hip_available() and scan_plan("fwd", 1, 1, 1, H) is not None


def lstm_v4_available(H: int, F: int) -> bool:
    """v4 fused-xW scan geometry: H <= 64, H%8==0, F%8==0, F<=128
    (the pad8 engine layout satisfies the alignment)."""
    return hip_available() and \
        scan_plan("fwd_fused", 1, 1, 1, H, F) is not None


def lstm_act_scan_available(H: int, F: int) -> bool:
    """Whether the engine's fused scans serve a non-tanh cell
    activation at this geometry. Only the v4 forward and the pipelined
    backward kernel take one, so both must apply."""
    return lstm_layer_mode(1, 1, H, F, "relu") == "fused"


def lstm_seq_fwd(xW, Wh):
    """Fused on-device LSTM sequence scan (GPU only), by the planner's
    public route: the pipelined v3 kernel for the barriered H <= 64
    layout, the barrier-free v2 kernel for H % 16 == 0 once its grid
    fills the chip, the big-H kernels for 64 < H <= 256;
    ``GORDO_LSTM_V1=1`` takes the unpipelined v1 / v2 entry."""
    return _require_hip().lstm_seq_fwd(xW, Wh, "fwd")


def lstm_seq_fwd_fused(xseq, Wx, Wh, bias, store_aux=True, act="tanh"):
    """v4 scan: the x-side gate GEMM runs INSIDE the recurrence over an
    LDS-resident [Wh ; Wx] tile — no xW round trip through HBM (the
    fleet's scans are bandwidth-bound). ``store_aux=False`` skips the
    cs/gacts stores for inference. GORDO_LSTM_V4=0 falls back to the
    two-step path at the engine level. ``act`` is the cell activation
    (tanh/relu/sigmoid/linear) of the candidate gate and of φ(c)."""
    act = act_code(act)
    if _on_gpu(xseq):
        return _require_hip().lstm_seq_fwd_fused(
            xseq, Wx, Wh, bias, bool(store_aux), act
        )
    # CPU oracle: explicit xW then the per-timestep reference scan
    G, B, T, F = xseq.shape
    H = Wh.shape[1]
    gates_all = ref.grouped_linear_fwd(
        xseq.reshape(G, B * T, F), Wx, bias, ACT_LINEAR
    ).view(G, B, T, 4 * H)
    h = torch.zeros(G, B, H, dtype=xseq.dtype)
    c = torch.zeros(G, B, H, dtype=torch.float32)
    hs = torch.empty(G, B, T, H, dtype=xseq.dtype)
    cs = torch.empty(G, B, T, H, dtype=torch.float32)
    ga = torch.empty(G, B, T, 4 * H, dtype=xseq.dtype)
    for t in range(T):
        gates = gates_all[:, :, t] + torch.bmm(h, Wh)
        h, c, gact = ref.lstm_pointwise_fwd(gates, c, act)
        hs[:, :, t] = h
        cs[:, :, t] = c
        ga[:, :, t] = gact
    if store_aux:
        return [hs, cs, ga]
    return [hs]


def lstm_seq_fwd_v3(xW, Wh):
    """The pipelined forward scan, directly (for A/B tests)."""
    return _require_hip().lstm_seq_fwd(xW, Wh, "fwd_v3")


def _need_v2(name, H):
    if H % 16 != 0 or H > 64:
        raise ValueError(f"{name} needs H % 16 == 0 and H <= 64")


def lstm_seq_fwd_v2(xW, Wh):
    """The barrier-free v2 forward scan, directly (H % 16 == 0,
    H <= 64): the v1 entry takes v2 at any grid size, without the fill
    gate of ``lstm_seq_fwd``."""
    _need_v2("lstm_seq_fwd_v2", xW.shape[-1] // 4)
    return _require_hip().lstm_seq_fwd(xW, Wh, "fwd_v1")


def lstm_seq_bwd_v2(dSeq, gacts, cs, Wh, last_only):
    """The barrier-free v2 backward scan, directly (same geometry and
    purpose as ``lstm_seq_fwd_v2``)."""
    _need_v2("lstm_seq_bwd_v2", gacts.shape[-1] // 4)
    return _require_hip().lstm_seq_bwd(
        dSeq, gacts, cs, Wh, bool(last_only), "bwd_v1"
    )


def last_scan_launch() -> dict:
    """Which scan kernel this thread's last ``lstm_seq_*`` call
    launched: ``family`` (fwd_v1/v2/v3/v4/big, bwd_v1/v2/v3/v5/pipe/
    big), ``rows`` (row tile; 64 for v2), ``hf`` (H/16, v2 only, else
    None) and, for bwd_pipe only, ``has_dx`` / ``last_only`` (else
    None). Host-side record; ``family`` is "" before any launch."""
    return _record(*_require_hip().last_scan_launch())


def last_scan_activation() -> str:
    """Cell activation name of this thread's last scan launch (kept
    beside ``last_scan_launch``): "tanh" for every tanh-only family."""
    return _require_hip().last_scan_activation()


def lstm_seq_bwd(dSeq, gacts, cs, Wh, last_only, act="tanh"):
    """Fused on-device LSTM backward (BPTT) scan (GPU only), by the
    planner's public route: the same version dispatch as
    ``lstm_seq_fwd``, with the bottom-layer entry of ``lstm_seq_bwd_v3``
    in the place of v3. A non-tanh ``act`` goes straight to that entry:
    only the pipelined kernel behind it takes a cell activation."""
    return _require_hip().lstm_seq_bwd(
        dSeq, gacts, cs, Wh, bool(last_only), "bwd", act_code(act)
    )


def _lstm_seq_bwd_cpu(dSeq, gacts, cs, Wh, last_only, act):
    """fp32 per-timestep BPTT over the pointwise reference (CPU lane)."""
    G, B, T, H4 = gacts.shape
    H = H4 // 4
    WhT = Wh.transpose(1, 2)
    dh_carry = torch.zeros(G, B, H, dtype=gacts.dtype)
    dc = torch.zeros(G, B, H, dtype=cs.dtype)
    dG = torch.empty_like(gacts)
    zero_c = torch.zeros_like(cs[:, :, 0])
    for t in range(T - 1, -1, -1):
        dh = dh_carry
        if not last_only:
            dh = dh + dSeq[:, :, t]
        elif t == T - 1:
            dh = dh + dSeq
        c_prev = cs[:, :, t - 1] if t > 0 else zero_c
        dg, dc = ref.lstm_pointwise_bwd(
            dh, dc, gacts[:, :, t], cs[:, :, t], c_prev, act
        )
        dG[:, :, t] = dg
        dh_carry = torch.bmm(dg, WhT)
    return dG


def lstm_seq_bwd_fused(dSeq, gacts, cs, Wh, Wx, last_only, act="tanh"):
    """Reverse scan with the bwd-data GEMM fused in: returns (dG, dX)
    where dX = dG @ Wx^T computed per step against an LDS-resident WxT
    (no dG HBM re-read). Geometry: H<=64, F<=128. The planner takes the
    16-byte pipelined kernel where it applies, else the v5 kernel
    (bit-identical outputs); ``GORDO_LSTM_PIPE=0`` forces v5. A
    non-tanh ``act`` runs only on the pipelined kernel and raises
    elsewhere."""
    act = act_code(act)
    if _on_gpu(gacts):
        out = _require_hip().lstm_seq_bwd_fused(
            dSeq, gacts, cs, Wh, Wx, bool(last_only), act
        )
        return out[0], out[1]
    dG = _lstm_seq_bwd_cpu(dSeq, gacts, cs, Wh, last_only, act)
    G, B, T, H4 = gacts.shape
    dX = ref.grouped_linear_bwd_data(
        dG.view(G, B * T, H4), Wx
    ).view(G, B, T, Wx.shape[1])
    return dG, dX


def lstm_seq_bwd_v3(dSeq, gacts, cs, Wh, last_only, act="tanh"):
    """The bottom-layer backward scan, directly (for A/B tests): the
    16-byte pipelined kernel where the planner finds it applies, else
    the v3 kernel; ``GORDO_LSTM_PIPE=0`` forces v3. A non-tanh ``act``
    runs only on the pipelined kernel and raises elsewhere."""
    act = act_code(act)
    if not _on_gpu(gacts):
        return _lstm_seq_bwd_cpu(dSeq, gacts, cs, Wh, last_only, act)
    return _require_hip().lstm_seq_bwd(
        dSeq, gacts, cs, Wh, bool(last_only), "bwd_bottom", act
    )


def lstm_seq_bwd_fused_out(dSeq, gacts, cs, Wh, Wx, last_only, dG, dX,
                           act="tanh"):
    """``lstm_seq_bwd_fused`` (GPU only) writing into caller-provided
    contiguous, 16-byte-aligned bf16 ``dG`` [G,B,T,4H] and ``dX``
    [G,B,T,F] — lets tests place the outputs between guard regions."""
    _require_hip().lstm_seq_bwd_fused(
        dSeq, gacts, cs, Wh, Wx, bool(last_only), act_code(act), dG, dX
    )


def lstm_seq_bwd_v3_out(dSeq, gacts, cs, Wh, last_only, dG, act="tanh"):
    """``lstm_seq_bwd_v3`` (GPU only, H <= 64) into a caller-provided
    ``dG`` (same contract as ``lstm_seq_bwd_fused_out``)."""
    _require_hip().lstm_seq_bwd(
        dSeq, gacts, cs, Wh, bool(last_only), "bwd_bottom", act_code(act), dG
    )


def anomaly_score(out, y, scale, minv, feat_thr, agg_thr):
    """Fused serving-path anomaly scoring (GPU only; callers fall back
    to numpy/pandas on CPU — machine/model/anomaly/diff.py)."""
    return _require_hip().anomaly_score(out, y, scale, minv, feat_thr,
                                        float(agg_thr))


def trail_min_max(X, w: int):
    """Per-row ``rolling(w).min().max()`` (K10). GPU tensors run the
    HIP kernel; CPU falls back to the scipy O(n) path
    (machine/model/utils.trail_min_max)."""
    if _on_gpu(X):
        return _require_hip().trail_min_max(X, int(w))
    from ..machine.model.utils import trail_min_max as cpu_tmm
    import numpy as _np

    return torch.as_tensor(
        _np.atleast_1d(cpu_tmm(X.numpy().T, int(w))), dtype=torch.float32
    )


def windowed_quantile(X, w: int, q: float):
    """Per-row rolling(w).quantile(q) with pandas min_periods=w NaN
    semantics (K11; q=0.5 == the smm rolling median)."""
    if _on_gpu(X):
        return _require_hip().windowed_quantile(X, int(w), float(q))
    import pandas as _pd

    df = _pd.DataFrame(X.numpy().T)
    out = df.rolling(int(w)).quantile(float(q)).to_numpy().T[:, int(w) - 1:]
    return torch.as_tensor(out, dtype=torch.float32)


def row_quantile(X, q: float):
    """Per-row NaN-dropping linear-interpolated quantile (K12)."""
    if _on_gpu(X):
        return _require_hip().row_quantile(X, float(q))
    import numpy as _np

    # in double: on fp32 input numpy forms the position q*(n-1) in fp32
    return torch.as_tensor(
        _np.nanquantile(X.numpy().astype(_np.float64), float(q), axis=1),
        dtype=torch.float32,
    )


_SMOOTH_METHODS = {"smm": 0, "sma": 1, "ewma": 2}


def smooth(X, window: int, method: str):
    """Per-row smoothing of ``X`` [R, N] with pandas semantics, fp64
    [R, N] out (completes K11): ``"smm"`` is ``rolling(window)
    .median()``, ``"sma"`` ``rolling(window).mean()`` and ``"ewma"``
    ``ewm(span=window).mean()``. NaN and +-inf are missing values in
    all three. GPU tensors run the HIP kernels (csrc/smoothing.hip;
    ``window >= 1``, smm ``window <= 8192``); CPU tensors take the
    pandas expressions of ``DiffBasedAnomalyDetector._smoothing``."""
    if method not in _SMOOTH_METHODS:
        raise ValueError(
            f"Unknown smoothing method {method!r}: expected one of "
            f"{sorted(_SMOOTH_METHODS)}"
        )
    window = int(window)
    if _on_gpu(X):
        return _require_hip().smooth(X, window, _SMOOTH_METHODS[method])
    if window < 1:
        raise ValueError("window must be at least 1")
    import pandas as _pd

    df = _pd.DataFrame(X.numpy().T)
    if method == "smm":
        sm = df.rolling(window).median()
    elif method == "sma":
        sm = df.rolling(window).mean()
    else:
        sm = df.ewm(span=window).mean()
    import numpy as _np

    return torch.as_tensor(
        _np.ascontiguousarray(sm.to_numpy(dtype=_np.float64).T)
    )


def last_smooth_launch() -> dict:
    """What this thread's last GPU ``smooth`` call launched:
    ``method`` (smm/sma/ewma), ``family`` ("smm_slide", "sma_window",
    "ewma_scan"; "nan_fill" when ``window > n`` left nothing to launch
    for smm/sma, "empty" for an empty input), ``rows``, ``n`` and
    ``window``. Host-side record; ``family`` is "" before any call."""
    method, family, rows, n, window = _require_hip().last_smooth_launch()
    return {"method": method, "family": family, "rows": rows, "n": n,
            "window": window}


def lstm_pointwise_fwd(gates, c_prev, act="tanh"):
    act = act_code(act)
    if _on_gpu(gates):
        return _require_hip().lstm_pointwise_fwd(gates, c_prev, act)
    return ref.lstm_pointwise_fwd(gates, c_prev, act)


def lstm_pointwise_bwd(dh, dc_next, gact, c, c_prev, act="tanh"):
    act = act_code(act)
    if _on_gpu(dh):
        return _require_hip().lstm_pointwise_bwd(
            dh, dc_next, gact, c, c_prev, act
        )
    return ref.lstm_pointwise_bwd(dh, dc_next, gact, c, c_prev, act)
