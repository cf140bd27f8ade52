"""
Packed many-model trainers.

The MI355X-native answer to the reference's pod-per-model fan-out
(SURVEY.md §2.4): G same-architecture models train in lockstep as ONE
set of grouped tensors — weights ``[G, in, out]``, activations
``[G, B, F]`` — so every layer of every model in the pack is a single
grouped MFMA GEMM launch instead of thousands of tiny ones. Per-model
data, per-model losses, per-model optimizer state; one flat fp32
parameter buffer (+ bf16 compute mirror on GPU) per pack so the
optimizer is one fused kernel over the whole fleet shard.

Training math matches Keras (glorot-uniform kernels, orthogonal LSTM
recurrent kernels, unit forget-gate bias) and honours the spec's
compile settings: the loss is one of mse / mae / huber / logcosh
(``ops.loss_bwd``, which also counts the Keras ``accuracy`` metric) and
the optimizer one of Adam (+amsgrad) / SGD / RMSprop / Adagrad / Adamax
with Keras 3 defaults (``ops.optimizer_step``). The default is Adam with
bias correction and MSE — reference factories:
gordo/machine/model/factories/feedforward_autoencoder.py,
lstm_autoencoder.py.
"""
from __future__ import annotations

import logging
import math
import os
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import ops
from .compaction import ratio_from_env, should_compact
from .early_stop import EarlyStopState
from .spec import ModelSpec

logger = logging.getLogger(__name__)


class FitHistory(dict):
    """The history ``BasePack.fit`` returns: the rectangular
    ``{key: [[G values] per epoch]}`` dict, plus ``epochs_run``, the
    number of epochs each model itself trained for (its stopped epoch
    + 1 under early stopping, else the epochs of the fit). Rows past
    ``epochs_run[g]`` hold model g's frozen-weight values while model g
    still rides along in the pack, and NaN once the pack has been
    compacted to its live models; every consumer cuts them off.
    ``best_epoch`` (early stopping only) is each model's epoch of the
    best monitored value: the one ``restore_best_weights`` goes back
    to. ``compactions`` (early stopping only; ``[]`` when none
    happened) lists ``(epoch, G_before, G_after)`` for every time the
    fit went on in a smaller pack of its live models, ``epoch`` the
    0-based epoch after which it did."""

    epochs_run: Optional[List[int]] = None
    best_epoch: Optional[List[int]] = None
    compactions: Optional[List[Tuple[int, int, int]]] = None


def _compute_dtype(device: torch.device) -> torch.dtype:
    return torch.bfloat16 if device.type == "cuda" else torch.float32


def _pad8(n: int) -> int:
    return (int(n) + 7) & ~7


def pad_enabled(device) -> bool:
    """Feature/hidden dims are zero-padded to multiples of 8 on GPU
    (GORDO_PAD8=0 disables): bf16x8 = 16 bytes unlocks vectorized
    global staging loads in every grouped GEMM (guide G13 — scalar
    bf16 staging is a 2-2.5x tax), and padded hidden units are
    PROVABLY inert: zero weights + zero bias give g=φ(0)=0 so
    c=f*0+i*0=0 and h=o*φ(0)=0 forever, for every LSTM cell activation
    φ with φ(0)=0: tanh, relu and linear (relu'(0) is taken as 0 and
    the pad units' dc, dh are 0 whatever φ' is). It FAILS for sigmoid:
    σ(0)=0.5 makes pad units emit non-zero h, and the next layer's pad
    rows then receive gradient; an LSTMPack with a sigmoid layer whose
    dims would actually be padded therefore builds unpadded
    (``LSTMPack._declare_params``). All the pad units' gradients are
    exactly 0 (dc=dh=0 chains), so every supported optimizer keeps
    their weights at 0 (each update is a multiple of g or of a moment
    of g). Every supported loss is 0 with zero gradient at d=0, so pad
    output columns add nothing; only the mean needs the REAL element
    count (ops.loss_bwd real_f). CPU packs stay unpadded (they are the
    fp32 oracle)."""
    return (
        torch.device(device).type == "cuda"
        and os.environ.get("GORDO_PAD8", "1") != "0"
    )


def _glorot_uniform(shape, gen):
    fan_in, fan_out = shape[-2], shape[-1]
    limit = math.sqrt(6.0 / (fan_in + fan_out))
    return (torch.rand(shape, generator=gen, dtype=torch.float32) * 2 - 1) * limit


def _orthogonal(shape, gen):
    rows, cols = shape[-2], shape[-1]
    a = torch.randn((max(rows, cols), min(rows, cols)), generator=gen)
    q, r = torch.linalg.qr(a)
    q = q * torch.sign(torch.diagonal(r))
    if rows < cols:
        q = q.T
    return q[:rows, :cols].contiguous()


class _ParamStore:
    """One flat fp32 master buffer + grads + optimizer state (+ bf16
    compute mirror on GPU), carved into named [G, ...] views.

    The state slots keep their Adam names: ``m`` is slot 0 (Adam/Adamax
    first moment, SGD momentum, RMSprop mean square, Adagrad
    accumulator), ``v`` slot 1 (Adam second moment, Adamax infinity
    norm, RMSprop momentum); ``vhat`` exists only for Adam+amsgrad."""

    def __init__(self, device: torch.device, optimizer_kind: str = "adam",
                 optimizer_params: Optional[Dict[str, Any]] = None):
        self.device = device
        self.optimizer_kind = optimizer_kind
        if optimizer_params is None:
            from .spec import resolve_optimizer

            optimizer_params = resolve_optimizer(optimizer_kind)[1]
        self.optimizer_params = dict(optimizer_params)
        self.compute_dtype = _compute_dtype(device)
        self._shapes: List[Tuple[str, Tuple[int, ...]]] = []
        self.logical: Dict[str, Tuple[int, ...]] = {}
        self._offsets: Dict[str, Tuple[int, int]] = {}
        self._total = 0
        self.views: Dict[str, torch.Tensor] = {}
        self.cviews: Dict[str, torch.Tensor] = {}
        self.gviews: Dict[str, torch.Tensor] = {}
        self.step_count = 0
        # per-model early stopping: int32 [G] device mask of the models
        # that still train. None (the unmasked kernels run) until a fit
        # with early stopping and G > 1 sets it.
        self.active: Optional[torch.Tensor] = None
        self._segments: Optional[torch.Tensor] = None
        # weight regularizers: (l1, l2) per declared tensor, and the
        # float32 [2, S] device table built from them on first use
        self._regs: Dict[str, Tuple[float, float]] = {}
        self._reg_table: Optional[torch.Tensor] = None
        # [G] penalty at the weights the latest optimizer_step started
        # from (the weights that batch's forward pass used)
        self.last_penalty: Optional[torch.Tensor] = None

    def declare(self, name: str, shape: Tuple[int, ...],
                logical: Optional[Tuple[int, ...]] = None,
                reg: Tuple[float, float] = (0.0, 0.0)):
        """``reg``: the (l1, l2) weight-regularizer coefficients of this
        tensor (l1 sum|w| + l2 sum w^2 joins the model's loss)."""
        n = int(np.prod(shape))
        self._offsets[name] = (self._total, n)
        self._shapes.append((name, shape))
        self.logical[name] = tuple(logical) if logical else tuple(shape)
        self._regs[name] = (float(reg[0]), float(reg[1]))
        self._total += n

    def allocate(self):
        dev = self.device
        self.p32 = torch.zeros(self._total, dtype=torch.float32, device=dev)
        self.g32 = torch.zeros(self._total, dtype=torch.float32, device=dev)
        self.m = torch.zeros(self._total, dtype=torch.float32, device=dev)
        self.v = torch.zeros(self._total, dtype=torch.float32, device=dev)
        self.vhat = (
            torch.zeros(self._total, dtype=torch.float32, device=dev)
            if self.optimizer_kind == "adam"
            and self.optimizer_params.get("amsgrad")
            else None
        )
        self._init_slots()
        self.plp = (
            torch.zeros(self._total, dtype=self.compute_dtype, device=dev)
            if self.compute_dtype != torch.float32
            else None
        )
        # device-resident optimizer step counter (hipGraph-capturable)
        self.step_buf = (
            torch.zeros(1, dtype=torch.int32, device=dev)
            if dev.type == "cuda"
            else None
        )
        for name, shape in self._shapes:
            off, n = self._offsets[name]
            self.views[name] = self.p32[off : off + n].view(*shape)
            self.gviews[name] = self.g32[off : off + n].view(*shape)
            self.cviews[name] = (
                self.plp[off : off + n].view(*shape)
                if self.plp is not None
                else self.views[name]
            )

    @property
    def segments(self) -> torch.Tensor:
        """Segment table of the flat buffer for the masked ops: tensor
        s is [G, per_s] at off_s, so model g owns off_s + g*per_s
        onwards. Built once, when a fit first needs it: a pack that
        never stops a model early uploads nothing."""
        if self._segments is None:
            self._segments = ops.segment_table(
                [self._offsets[name][0] for name, _ in self._shapes],
                [self._offsets[name][1] // max(int(shape[0]), 1)
                 for name, shape in self._shapes],
                self.device,
            )
        return self._segments

    @property
    def regularized(self) -> bool:
        return any(l1 or l2 for l1, l2 in self._regs.values())

    @property
    def reg_table(self) -> Optional[torch.Tensor]:
        """float32 [2, S] coefficient table beside ``segments`` (l1
        row, l2 row), built once; None when every coefficient is zero:
        such a store steps and reports exactly as one without
        regularizers."""
        if self._reg_table is None and self.regularized:
            self._reg_table = ops.reg_table(
                [self._regs[name][0] for name, _ in self._shapes],
                [self._regs[name][1] for name, _ in self._shapes],
                self.device,
            )
        return self._reg_table

    def weight_penalty(self) -> Optional[torch.Tensor]:
        """[G] penalty of the current weights; None without
        regularizers."""
        reg = self.reg_table
        if reg is None:
            return None
        return ops.weight_penalty(
            self.p32, self.segments, reg, self.n_models
        )

    def set_active(self, active) -> None:
        """Upload the [G] mask of the models that still train (None:
        back to the unmasked step)."""
        self.active = (
            None if active is None else self.model_mask(active)
        )

    def model_mask(self, mask) -> torch.Tensor:
        """A host bool [G] mask as the int32 device tensor the masked
        ops take."""
        return torch.as_tensor(
            np.asarray(mask, dtype=np.int32), device=self.device
        )

    def copy_models(self, dst: torch.Tensor, src: torch.Tensor, mask,
                    mirror: bool = False) -> None:
        """dst <- src for the flat-buffer slices of the masked models;
        ``mirror`` also refreshes their slices of the bf16 mirror."""
        ops.masked_copy(
            dst, src, self.model_mask(mask), self.segments,
            self.plp if mirror else None,
        )

    # -- pack compaction: whole models between stores of different G --
    @property
    def n_models(self) -> int:
        return int(self._shapes[0][1][0])

    def segments_for(self, G: int) -> torch.Tensor:
        """Segment table of this store's tensors laid out for G models
        (the flat buffer is the declared tensors one after the other,
        so tensor s starts at sum_{k<s} G * per_k)."""
        per = [
            self._offsets[name][1] // self.n_models
            for name, _ in self._shapes
        ]
        offsets = np.concatenate(([0], np.cumsum(per)[:-1])) * int(G)
        return ops.segment_table(offsets.tolist(), per, self.device)

    def gathered_p32(self, live) -> torch.Tensor:
        """A new flat parameter buffer that holds this store's models
        ``live``, in that order, laid out for ``len(live)`` models."""
        live = [int(g) for g in live]
        out = torch.empty(
            self._total // self.n_models * len(live),
            dtype=torch.float32, device=self.device,
        )
        ops.remap_models(
            out, self.p32, list(range(len(live))), live,
            self.segments_for(len(live)), self.segments,
            len(live), self.n_models,
        )
        return out

    def _move_models(self, dst: "_ParamStore", dst_index, src_index,
                     extra=None) -> None:
        """Models ``src_index`` of this store become models
        ``dst_index`` of ``dst``: parameters (and dst's bf16 mirror, in
        the same launch), every optimizer slot and, as ``extra = (dst
        buffer, src buffer)``, one more buffer of the same layout. The
        step counter carries over: every model that moves took every
        step, which is also why the masked step shares one counter."""
        args = (dst_index, src_index, dst.segments, self.segments,
                dst.n_models, self.n_models)
        ops.remap_models(dst.p32, self.p32, *args, dst_lp=dst.plp)
        for (_k, d), (_k2, s) in zip(dst.slots(), self.slots()):
            ops.remap_models(d, s, *args)
        if extra is not None:
            ops.remap_models(extra[0], extra[1], *args)
        dst.step_count = self.step_count
        if dst.step_buf is not None:
            dst.step_buf.copy_(self.step_buf)

    def gather_models(self, child: "_ParamStore", live, extra=None) -> None:
        """``child``'s models 0, 1, ... <- this store's models ``live``
        (``extra``: (child's buffer, this store's))."""
        live = [int(g) for g in live]
        self._move_models(child, list(range(len(live))), live, extra)

    def scatter_models(self, child: "_ParamStore", live, extra=None) -> None:
        """This store's models ``live`` <- ``child``'s models 0, 1, ...
        (``extra``: (this store's buffer, child's)); the other models
        of this store keep their bits."""
        live = [int(g) for g in live]
        child._move_models(self, live, list(range(len(live))), extra)

    def sync_lp(self):
        if self.plp is not None:
            self.plp.copy_(self.p32)

    def zero_grad(self):
        self.g32.zero_()

    def adam_step(self, lr, beta1, beta2, eps):
        self.step_count += 1
        ops.adam_step(
            self.p32, self.g32, self.m, self.v,
            lr, beta1, beta2, eps, self.step_count, self.plp,
            step_buf=self.step_buf,
        )

    def optimizer_step(self):
        """One step of the spec's optimizer over the whole buffer, or,
        while ``active`` is set, over the models that still train."""
        self.step_count += 1
        reg = self.reg_table
        if reg is not None:
            # the penalty belongs to the loss of this batch, at the
            # weights its forward pass used: before they move. The step
            # is the segment-aware one, with or without a mask.
            self.last_penalty = self.weight_penalty()
            ops.optimizer_step(
                self.optimizer_kind, self.p32, self.g32, self.m, self.v,
                self.vhat, self.optimizer_params, self.step_count, self.plp,
                step_buf=self.step_buf, active=self.active,
                segments=self.segments, reg=reg, G=self.n_models,
            )
            return
        # active None (no early stopping, or G = 1): the unmasked kernels
        ops.optimizer_step(
            self.optimizer_kind, self.p32, self.g32, self.m, self.v,
            self.vhat, self.optimizer_params, self.step_count, self.plp,
            step_buf=self.step_buf, active=self.active,
            segments=None if self.active is None else self.segments,
        )

    def _init_slots(self):
        if self.optimizer_kind == "adagrad":
            self.m.fill_(
                float(self.optimizer_params["initial_accumulator_value"])
            )
        else:
            self.m.zero_()
        self.v.zero_()
        if self.vhat is not None:
            self.vhat.zero_()

    def slots(self) -> List[Tuple[str, torch.Tensor]]:
        """(key prefix, flat state tensor) for every slot that exists."""
        out = [("m", self.m), ("v", self.v)]
        if self.vhat is not None:
            out.append(("vhat", self.vhat))
        return out

    def reset_adam(self):
        """Reset the optimizer state (whatever the optimizer)."""
        self._init_slots()
        self.step_count = 0
        if self.step_buf is not None:
            self.step_buf.zero_()


class BasePack:
    def __init__(self, spec: ModelSpec, G: int, device=None, seeds=None,
                 init_p32: Optional[torch.Tensor] = None):
        self.spec = spec
        self.G = G
        self.device = torch.device(
            device if device is not None else
            ("cuda" if torch.cuda.is_available() else "cpu")
        )
        self.store = _ParamStore(
            self.device, spec.optimizer_kind, spec.optimizer_params
        )
        self._loss_kind = spec.loss_kind
        self._loss_delta = float(spec.loss_params.get("delta", 1.0))
        # per-model Keras "accuracy" hit count of the latest train_batch
        self.last_correct: Optional[torch.Tensor] = None
        self.pad8 = pad_enabled(self.device)
        self._pad = _pad8 if self.pad8 else (lambda n: int(n))
        # per-param custom logical<->physical converters (LSTM gate
        # interleave); default is plain dim slicing by store.logical
        self._extractors: Dict[str, Any] = {}
        self.seeds = list(seeds) if seeds is not None else list(range(G))
        assert len(self.seeds) == G
        self._declare_params()
        self.store.allocate()
        if init_p32 is not None:
            # clone-init: copy a sibling pack's flat parameter snapshot
            # (per-model glorot + orthogonal QR costs ~1 s per pack)
            self.store.p32.copy_(init_p32)
        else:
            self._init_weights()
        self.store.sync_lp()

    # -- interface -------------------------------------------------------
    def _declare_params(self):
        raise NotImplementedError

    def _init_weights(self):
        raise NotImplementedError

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def train_batch(self, Xb, Tb) -> torch.Tensor:
        raise NotImplementedError

    def eval_batch_stats(self, Xb, Tb) -> Tuple[torch.Tensor, torch.Tensor]:
        """Forward-only (per-model configured loss, accuracy hit count)
        for a gathered batch (the validation pass of fit)."""
        raise NotImplementedError

    def eval_batch(self, Xb, Tb) -> torch.Tensor:
        """Forward-only per-model loss for a gathered batch."""
        return self.eval_batch_stats(Xb, Tb)[0]

    def _loss_bwd(self, Y, Tb, want_grad: bool = True):
        """The spec's loss over [G, B, F_physical] outputs/targets:
        (loss[G], dY | None, correct[G]); means divide by the LOGICAL
        width (pad diffs are exactly 0 and every loss is 0 at 0)."""
        return ops.loss_bwd(
            Y, Tb.to(Y.dtype), self._loss_kind, self._logical_out,
            self._loss_delta, want_grad,
        )

    # -- common ----------------------------------------------------------
    @property
    def compute_dtype(self):
        return self.store.compute_dtype

    def _to_compute(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(device=self.device, dtype=self.compute_dtype)

    def _pad_io(self, Xb, Tb):
        """Defensive padding for DIRECT train_batch/eval_batch calls
        (fit() pads the whole series up front; callers like profiling
        harnesses or graph capture may pass logical-width tensors)."""
        if self.pad8:
            if Xb.shape[-1] == self._logical_in:
                Xb = self._pad_features(Xb, self._logical_in)
            if Tb is not None and Tb.shape[-1] == self._logical_out:
                Tb = self._pad_features(Tb, self._logical_out)
        return Xb, Tb

    def _pad_features(self, t: torch.Tensor, logical_f: int) -> torch.Tensor:
        """Zero-pad the last (feature) dim to the physical width."""
        pf = self._pad(logical_f)
        if t.shape[-1] == pf:
            return t
        assert t.shape[-1] == logical_f, (t.shape, logical_f)
        return torch.nn.functional.pad(t, (0, pf - logical_f))

    def param_names(self) -> List[str]:
        return [name for name, _ in self.store._shapes]

    def _extract_logical(self, name: str, arr: np.ndarray) -> np.ndarray:
        """Physical [per-model] array -> logical (serialized) layout."""
        ex = self._extractors.get(name)
        if ex is not None:
            return ex[0](arr)
        logical = self.store.logical[name][1:]
        if arr.shape == tuple(logical):
            return arr.copy()
        return arr[tuple(slice(0, d) for d in logical)].copy()

    def _insert_logical(self, name: str, view: torch.Tensor,
                        arr: np.ndarray):
        """Write a logical array into the physical [per-model] view
        (pad regions stay zero)."""
        ex = self._extractors.get(name)
        t = torch.from_numpy(np.ascontiguousarray(arr))
        if ex is not None:
            ex[1](view, t)
            return
        logical = self.store.logical[name][1:]
        if tuple(view.shape) == tuple(logical):
            view.copy_(t)
            return
        view.zero_()
        view[tuple(slice(0, d) for d in logical)].copy_(t)

    def state_for_model(self, g: int) -> Dict[str, np.ndarray]:
        return {
            name: self._extract_logical(
                name, self.store.views[name][g].detach().cpu().numpy()
            )
            for name in self.param_names()
        }

    def states_for_all_models(self) -> List[Dict[str, np.ndarray]]:
        """Per-model weight dicts via ONE device-to-host transfer of the
        flat parameter buffer (per-model-per-param .cpu() slices cost
        ~1 s per 62-model pack)."""
        flat = self.store.p32.detach().cpu().numpy()
        out: List[Dict[str, np.ndarray]] = [dict() for _ in range(self.G)]
        for name, shape in self.store._shapes:
            off, n = self.store._offsets[name]
            arr = flat[off : off + n].reshape(shape)
            for g in range(self.G):
                out[g][name] = self._extract_logical(name, arr[g])
        return out

    def load_model_state(self, g: int, state: Dict[str, np.ndarray]):
        for name, arr in state.items():
            self._insert_logical(
                name, self.store.views[name][g], np.asarray(arr)
            )
        self.store.sync_lp()

    def optimizer_state_for_model(self, g: int) -> Dict[str, np.ndarray]:
        out = {}
        for name in self.param_names():
            off, n = self.store._offsets[name]
            shape = self.store.views[name].shape
            for prefix, slot in self.store.slots():
                out[prefix + ":" + name] = (
                    slot[off : off + n].view(*shape)[g].cpu().numpy().copy()
                )
        return out

    # ---- the epoch loop ------------------------------------------------
    # hipGraph capture of the steady-state train_batch: the whole
    # fwd+bwd+Adam kernel sequence replays as ONE graph launch per
    # full-size batch (shapes static; the shuffled gather runs eagerly
    # into static buffers; the ragged last batch stays eager).
    # OPT-IN (GORDO_HIPGRAPH=1): measured perf-neutral on this workload
    # (it is GPU-bound, not launch-bound), and torch-ROCm's CUDAGraph
    # destructor intermittently aborts the process with "The graph
    # should be registered to the state" (HIPGeneratorImpl.cpp:158)
    # when graphs are garbage-collected in long multi-pack processes.
    _graph_enabled = True  # env re-checked per step; instance sets
    # this False permanently after a capture failure
    # hip stream-capture mode is process-global: captures from two
    # threads at once crash the process. One capture at a time.
    _graph_capture_lock = __import__("threading").Lock()

    def _graph_train_step(self, Xb: torch.Tensor, Tb: torch.Tensor):
        """Replay (capturing on first use) the train_batch graph for
        this batch shape. Returns the live loss tensor, or None when
        capture is unavailable for this configuration."""
        if not (
            self._graph_enabled
            and os.environ.get("GORDO_HIPGRAPH", "0") == "1"
            and self.device.type == "cuda"
            # a masked step (per-model early stopping) runs eagerly
            and self.store.active is None
            # so does a regularized one: its step is the segment-aware
            # kernel too, and the penalty launch is not captured
            and not self.store.regularized
        ):
            # _graph_enabled False (set per-instance after a capture
            # failure) wins; otherwise the env is re-read so flipping
            # GORDO_HIPGRAPH at runtime takes effect
            return None
        key = (tuple(Xb.shape), tuple(Tb.shape))
        cached = getattr(self, "_graph_cache", None)
        if cached is None:
            cached = self._graph_cache = {}
        entry = cached.get(key)
        if entry is None:
            if len(cached) >= 4:  # bound distinct shapes per pack
                return None
            try:
                # flush pending GC NOW: a garbage pack's CUDAGraph
                # destructor running inside the upcoming capture (or
                # inside another thread's capture) hits HIP's
                # generator-state unregister check and terminates the
                # process
                import gc

                gc.collect()
                sx = torch.empty_like(Xb)
                st = torch.empty_like(Tb)
                sx.copy_(Xb)
                st.copy_(Tb)
                # warmup + capture run real optimizer steps — snapshot
                # the training state and restore it afterwards so
                # capture does not perturb the training trajectory.
                store = self.store
                snap = (
                    store.p32.clone(),
                    [slot.clone() for _k, slot in store.slots()],
                    store.step_buf.clone(), store.step_count,
                )
                with BasePack._graph_capture_lock:
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s):
                        self.train_batch(sx, st)
                    torch.cuda.current_stream().wait_stream(s)
                    graph = torch.cuda.CUDAGraph()
                    # thread_local: other builder threads keep launching
                    # on their own streams while this one captures
                    with torch.cuda.graph(
                        graph, capture_error_mode="thread_local"
                    ):
                        loss = self.train_batch(sx, st)
                        correct = self.last_correct
                store.p32.copy_(snap[0])
                for (_k, slot), saved in zip(store.slots(), snap[1]):
                    slot.copy_(saved)
                store.step_buf.copy_(snap[2])
                store.step_count = snap[3]
                store.sync_lp()
                entry = cached[key] = (graph, sx, st, loss, correct)
            except Exception:
                logger.warning(
                    "hipGraph capture failed; falling back to eager",
                    exc_info=True,
                )
                self._graph_enabled = False
                return None
        graph, sx, st, loss, correct = entry
        sx.copy_(Xb)
        st.copy_(Tb)
        graph.replay()
        self.store.step_count += 1  # device step_buf is the truth
        self.last_correct = correct
        return loss

    def release_graphs(self):
        """Drop captured graphs deterministically (outside any capture)
        instead of at arbitrary GC time."""
        for attr in ("_graph_cache", "_pred_graph_cache"):
            cached = getattr(self, attr, None)
            if cached:
                with BasePack._graph_capture_lock:
                    cached.clear()

    def predict_captured(self, X: torch.Tensor) -> torch.Tensor:
        """hipGraph-replayed inference forward for static request shapes
        (the serving hot path: north-star "batched anomaly inference on
        hipGraph-captured steps"). Each distinct input shape captures
        once and replays thereafter — one graph launch instead of one
        host launch per layer. Opt-in via ``GORDO_SERVE_HIPGRAPH=1``
        (the torch-ROCm graph-destructor abort makes capture opt-in
        everywhere — ROADMAP); anything unexpected falls back to the
        eager predict. Thread-safe: replay + readout under a per-pack
        lock (the static buffers are shared)."""
        if not (
            os.environ.get("GORDO_SERVE_HIPGRAPH", "0") == "1"
            and self.device.type == "cuda"
            and self._graph_enabled
        ):
            return self.predict(X)
        Xc = self._to_compute(X)
        key = tuple(Xc.shape)
        lock = getattr(self, "_pred_graph_lock", None)
        if lock is None:
            lock = self._pred_graph_lock = __import__("threading").Lock()
        with lock:
            cached = getattr(self, "_pred_graph_cache", None)
            if cached is None:
                cached = self._pred_graph_cache = {}
            entry = cached.get(key)
            if entry is None:
                if len(cached) >= 8:  # bound distinct request shapes
                    return self.predict(Xc)
                try:
                    import gc

                    gc.collect()  # same destructor hazard as train capture
                    with BasePack._graph_capture_lock:
                        sx = Xc.clone()
                        s = torch.cuda.Stream()
                        s.wait_stream(torch.cuda.current_stream())
                        with torch.cuda.stream(s), torch.no_grad():
                            self.predict(sx)
                        torch.cuda.current_stream().wait_stream(s)
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(
                            graph, capture_error_mode="thread_local"
                        ), torch.no_grad():
                            out = self.predict(sx)
                    entry = cached[key] = (graph, sx, out)
                except Exception:
                    logger.warning(
                        "serving hipGraph capture failed; staying eager",
                        exc_info=True,
                    )
                    self._graph_enabled = False
                    return self.predict(Xc)
            graph, sx, out = entry
            sx.copy_(Xc)
            graph.replay()
            # clone before releasing the lock: the static out buffer is
            # overwritten by the next replay
            return out.clone()

    def fit(
        self,
        X: torch.Tensor,
        Y: torch.Tensor,
        epochs: int = 1,
        batch_size: int = 256,
        shuffle: bool = True,
        verbose: int = 0,
        early_stopping: Optional[Dict[str, Any]] = None,
        validation_split: float = 0.0,
        **_,
    ) -> Dict[str, list]:
        """
        Train the whole pack. X: [G, N, F_in] (already on device),
        Y: [G, N, F_out]. Returns a Keras-style history dict with
        per-model per-epoch values: {"loss": [[...G...] per epoch],
        "accuracy": ...}. ``loss`` is the spec's configured loss and
        ``accuracy`` the Keras metric of that name (argmax agreement
        per row; binary accuracy for one output column), accumulated
        over the epoch's batches as Keras does. ``early_stopping``
        (``engine.early_stop``) stops every model at its own patience;
        the returned ``FitHistory`` says in ``epochs_run`` how many
        epochs each model trained for.
        """
        if self.pad8:
            X = self._pad_features(X, self._logical_in)
            Y = self._pad_features(Y, self._logical_out)
        G, N = X.shape[0], X.shape[1]
        history = FitHistory({"loss": [], "accuracy": []})
        n_all = self._n_samples(N)
        # keras validation_split semantics: the LAST fraction of samples
        # (in input order, before shuffling) is held out; history gains
        # val_loss/val_accuracy and EarlyStopping can monitor val_loss
        n_train = n_all
        if validation_split and validation_split > 0.0:
            n_train = int(n_all * (1.0 - float(validation_split)))
            n_train = max(1, min(n_train, n_all))
            if n_train < n_all:
                history["val_loss"] = []
                history["val_accuracy"] = []
        # EarlyStopping (the Keras rule, engine/early_stop.py): every
        # model stops at its OWN patience. A stopped model still runs
        # forward and backward in lockstep with the pack, but the masked
        # optimizer step leaves its parameters, optimizer state and
        # mirror alone, so its weights are those of a solo fit. Once
        # few enough models are left (engine/compaction.py) the fit
        # goes on in a child pack of the live models only, which is
        # scattered back into this one. The fit ends when every model
        # has ended.
        es: Optional[EarlyStopState] = None
        compact_ratio: Optional[float] = None
        if early_stopping is not None:
            es = EarlyStopState(G, early_stopping)
            compact_ratio = ratio_from_env()
            history.compactions = []
            if G > 1:
                self.store.set_active(np.ones(G, dtype=bool))
        try:
            epochs_done = self._fit_epochs(
                X, Y, epochs, batch_size, shuffle, verbose, history,
                n_train, n_all, es, compact_ratio,
            )
        finally:
            self.store.set_active(None)
        if es is None:
            history.epochs_run = [epochs_done] * G
        else:
            history.epochs_run = [
                int(es.stopped_epoch[g]) + 1 if es.ended[g] else epochs_done
                for g in range(G)
            ]
            history.best_epoch = [int(e) for e in es.best_epoch]
        return history

    def _fit_epochs(self, X, Y, epochs, batch_size, shuffle, verbose,
                    history, n_train, n_all, es,
                    compact_ratio: Optional[float] = None) -> int:
        """The epoch loop of ``fit``; returns the number of epochs run.

        ``cur`` is the pack that trains: this one, or, after a
        compaction, a child pack whose model j is this pack's model
        ``live[j]``. Early-stopping state, history rows and the shuffle
        generators stay indexed by this pack's models."""
        G = X.shape[0]
        n_val = n_all - n_train
        n_batches = max(1, math.ceil(n_train / batch_size))
        # one generator per model of THIS pack: a live model's stream
        # goes on across a compaction
        gens = [torch.Generator().manual_seed(int(s) & 0x7FFFFFFF) for s in self.seeds]
        cur: BasePack = self
        live = np.arange(G)
        Xc, Yc = X, Y  # cur's rows of the padded series
        # best weights: best_p32 in this pack's layout, cur_best in
        # cur's (the same buffer while cur is this pack)
        best_p32: Optional[torch.Tensor] = None
        cur_best: Optional[torch.Tensor] = None
        epochs_done = 0

        def row(values):
            """A [G] history row from cur's per-model values."""
            if cur is self:
                return values
            out = [math.nan] * G
            for j, g in enumerate(live):
                out[g] = values[j]
            return out

        try:
            for epoch in range(epochs):
                epochs_done = epoch + 1
                Gc = cur.G
                if shuffle:
                    perm = torch.stack(
                        [torch.randperm(n_train, generator=gens[g])
                         for g in live]
                    ).to(self.device)
                else:
                    perm = (
                        torch.arange(n_train, device=self.device)
                        .unsqueeze(0)
                        .expand(Gc, -1)
                    )
                epoch_loss = torch.zeros(
                    Gc, dtype=torch.float32, device=self.device
                )
                epoch_correct = torch.zeros(
                    Gc, dtype=torch.float32, device=self.device
                )
                samples_seen = 0
                for b in range(n_batches):
                    idx = perm[:, b * batch_size : (b + 1) * batch_size]
                    if idx.shape[1] == 0:
                        continue
                    Xb, Tb = cur._gather_batch(Xc, Yc, idx)
                    loss = cur._graph_train_step(Xb, Tb)
                    if loss is None:
                        loss = cur.train_batch(Xb, Tb)
                    if cur.store.regularized:
                        # Keras reports data loss + weight penalty
                        loss = loss + cur.store.last_penalty
                    epoch_loss += loss * idx.shape[1]
                    epoch_correct += cur.last_correct
                    samples_seen += idx.shape[1]
                # loss and accuracy leave the device together: one
                # transfer
                epoch_stats = torch.stack(
                    [epoch_loss, epoch_correct]
                ) / max(samples_seen, 1)
                epoch_loss, epoch_acc = epoch_stats.cpu().tolist()
                history["loss"].append(row(epoch_loss))
                history["accuracy"].append(row(epoch_acc))
                if n_val > 0:
                    val_loss = torch.zeros(
                        Gc, dtype=torch.float32, device=self.device
                    )
                    val_correct = torch.zeros(
                        Gc, dtype=torch.float32, device=self.device
                    )
                    vseen = 0
                    for vs_ in range(n_train, n_all, batch_size):
                        vidx = (
                            torch.arange(
                                vs_, min(vs_ + batch_size, n_all),
                                device=self.device,
                            ).unsqueeze(0).expand(Gc, -1)
                        )
                        Xvb, Tvb = cur._gather_batch(Xc, Yc, vidx)
                        vl, vc = cur.eval_batch_stats(Xvb, Tvb)
                        val_loss += vl * vidx.shape[1]
                        val_correct += vc
                        vseen += vidx.shape[1]
                    val_stats = (
                        torch.stack([val_loss, val_correct]) / max(vseen, 1)
                    )
                    # once per validation pass: the weights do not move
                    val_penalty = cur.store.weight_penalty()
                    if val_penalty is not None:
                        val_stats[0] += val_penalty
                    val_losses, val_acc = val_stats.cpu().tolist()
                    history["val_loss"].append(row(val_losses))
                    history["val_accuracy"].append(row(val_acc))
                if verbose:
                    logger.info(
                        "epoch %d/%d mean-loss=%.6g", epoch + 1, epochs,
                        float(np.nanmean(epoch_loss)),
                    )
                if es is None:
                    continue
                # a compacted-out model's NaN never improves, and ended
                # models are outside the rule anyway
                upd = es.update(epoch, es.monitored(history))
                if upd.capture.any():
                    # best weights of the models that improved
                    if cur_best is None:
                        cur_best = torch.empty_like(cur.store.p32)
                        if cur is self:
                            best_p32 = cur_best
                    cur.store.copy_models(
                        cur_best, cur.store.p32, upd.capture[live]
                    )
                if upd.stop.any():
                    cur._restore_best(
                        cur_best, (upd.stop & es.has_best)[live]
                    )
                    if verbose:
                        logger.info(
                            "early stopping at epoch %d/%d: models %s",
                            epoch + 1, epochs,
                            np.nonzero(upd.stop)[0].tolist(),
                        )
                    if es.ended.all():
                        break
                    n_live = int((~es.ended).sum())
                    if (
                        compact_ratio is not None
                        and epoch + 1 < epochs
                        and should_compact(Gc, n_live, compact_ratio)
                    ):
                        # one hop is one simple mapping: the current
                        # child goes back into this pack first, the
                        # next one is gathered from this pack
                        if cur is not self:
                            best_p32 = self._absorb_child(
                                cur, live, best_p32, cur_best
                            )
                            cur = self
                            cur_best = None  # the child's buffers go
                        live = np.nonzero(~es.ended)[0]
                        cur, cur_best = self._live_child(live, best_p32)
                        sel = torch.as_tensor(live, device=X.device)
                        Xc = X.index_select(0, sel)
                        Yc = Y.index_select(0, sel)
                        history.compactions.append((epoch, Gc, cur.G))
                        if verbose:
                            logger.info(
                                "pack compacted after epoch %d/%d: %d -> "
                                "%d models", epoch + 1, epochs, Gc, cur.G,
                            )
                    elif Gc > 1:  # the mask changed: upload it
                        cur.store.set_active((~es.ended)[live])
            if es is not None:
                # models that ran to the epoch cap end here
                cur._restore_best(cur_best, (~es.ended & es.has_best)[live])
            if cur is not self:
                self._absorb_child(cur, live, None, None)
                cur = self
        finally:
            if cur is not self:  # an error inside a child's epoch
                cur.release_graphs()
        return epochs_done

    def _live_child(self, live, best_p32):
        """A pack of this pack's models ``live`` alone, in the state
        they are in: parameters, mirror, optimizer slots, step counter
        and (when held) best weights. Returns (child, its best-weights
        buffer or None). Built from the gathered parameters, so no
        weights are drawn; it decides ``_use_fused`` with its own G."""
        child = type(self)(
            self.spec, len(live), device=self.device,
            seeds=[self.seeds[g] for g in live],
            init_p32=self.store.gathered_p32(live),
        )
        assert (
            child.store._total * self.G == self.store._total * child.G
        ), "a child pack must lay its models out as its parent does"
        child_best = None
        if best_p32 is not None:
            child_best = torch.empty_like(child.store.p32)
        self.store.gather_models(
            child.store, live,
            None if best_p32 is None else (child_best, best_p32),
        )
        # masked from its first batch, as fit starts this pack: the
        # train step is then never captured (nor re-captured) for G > 1
        if child.G > 1:
            child.store.set_active(np.ones(child.G, dtype=bool))
        return child, child_best

    def _absorb_child(self, child, live, best_p32, child_best):
        """Scatter ``child`` back into this pack's models ``live`` and
        drop it. With ``child_best`` its best weights go back too;
        returns this pack's best-weights buffer."""
        extra = None
        if child_best is not None:
            if best_p32 is None:
                best_p32 = torch.empty_like(self.store.p32)
            extra = (best_p32, child_best)
        self.store.scatter_models(child.store, live, extra)
        # captured graphs (a G = 1 child may hold one) go now, not at
        # some later garbage collection
        child.release_graphs()
        return best_p32

    def _restore_best(self, best_p32, mask) -> None:
        """The masked models' weights (and mirror) become their best
        weights; optimizer state is not restored."""
        if best_p32 is not None and mask.any():
            self.store.copy_models(
                self.store.p32, best_p32, mask, mirror=True
            )

    def _n_samples(self, N: int) -> int:
        return N

    def _gather_batch(self, X, Y, idx):
        G, F = X.shape[0], X.shape[2]
        Fo = Y.shape[2]
        Xb = X.gather(1, idx.unsqueeze(-1).expand(G, idx.shape[1], F))
        Tb = Y.gather(1, idx.unsqueeze(-1).expand(G, idx.shape[1], Fo))
        return Xb, Tb


class DensePack(BasePack):
    """Grouped feedforward autoencoder trainer (kernels K1-K4 of
    SURVEY.md §2.3)."""

    def _declare_params(self):
        dims = self.spec.dense_dims()
        self.layer_meta_logical = dims
        p = self._pad
        # physical layer dims padded to 8 (pad units provably inert —
        # see pad_enabled); activations between layers inherit the
        # padded widths so every grouped GEMM stages 16-byte vectors
        self.layer_meta = [
            (p(fin), p(fout), act, l1) for fin, fout, act, l1 in dims
        ]
        self._logical_in = dims[0][0]
        self._logical_out = dims[-1][1]
        for i, (fin, fout, _act, _l1) in enumerate(self.layer_meta):
            lfin, lfout = dims[i][0], dims[i][1]
            regs = self.spec.layers[i].weight_regs()
            self.store.declare(f"W{i}", (self.G, fin, fout),
                               logical=(self.G, lfin, lfout),
                               reg=regs["kernel"])
            self.store.declare(f"b{i}", (self.G, fout),
                               logical=(self.G, lfout), reg=regs["bias"])

    def _init_weights(self):
        for g in range(self.G):
            gen = torch.Generator().manual_seed(int(self.seeds[g]) & 0x7FFFFFFF)
            for i, (lfin, lfout, _act, _l1) in enumerate(
                self.layer_meta_logical
            ):
                self.store.views[f"W{i}"][g][:lfin, :lfout].copy_(
                    _glorot_uniform((lfin, lfout), gen)
                )
                # biases stay zero

    def forward(self, X: torch.Tensor) -> List[torch.Tensor]:
        acts = [X]
        a = X
        for i, (_fin, _fout, act, _l1) in enumerate(self.layer_meta):
            a = ops.grouped_linear_fwd(
                a, self.store.cviews[f"W{i}"],
                self.store.views[f"b{i}"], act,
            )
            acts.append(a)
        return acts

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        Xc = self._to_compute(X)
        if self.pad8:
            Xc = self._pad_features(Xc, self._logical_in)
        out = self.forward(Xc)[-1]
        return out[..., : self._logical_out]

    def eval_batch_stats(self, Xb, Tb):
        Xb, Tb = self._pad_io(Xb, Tb)
        loss, _, correct = self._loss_bwd(
            self.forward(Xb)[-1], Tb, want_grad=False
        )
        return loss, correct

    def train_batch(self, Xb, Tb) -> torch.Tensor:
        Xb, Tb = self._pad_io(Xb, Tb)
        acts = self.forward(Xb)
        loss, dA, self.last_correct = self._loss_bwd(acts[-1], Tb)
        for i in range(len(self.layer_meta) - 1, -1, -1):
            _fin, _fout, act, l1 = self.layer_meta[i]
            dZ = ops.act_l1_bwd(dA, acts[i + 1], act, l1)
            dW, db = ops.grouped_linear_wgrad(acts[i], dZ)
            self.store.gviews[f"W{i}"].copy_(dW)
            self.store.gviews[f"b{i}"].copy_(db)
            if i > 0:
                dA = ops.grouped_linear_bwd_data(dZ, self.store.cviews[f"W{i}"])
        self.store.optimizer_step()
        return loss


class LSTMPack(BasePack):
    """Grouped stacked-LSTM autoencoder/forecast trainer (kernels K5-K7).

    The sliding-window featurizer is zero-copy: windows are gathered
    straight out of the resident [G, N, F] series tensor (the device
    analog of create_keras_timeseriesgenerator, reference
    models.py:713-793)."""

    @staticmethod
    def _gate_converters(H, pH, row_l):
        """Logical<->physical converters for gate-interleaved LSTM
        params: physical gate blocks are pH wide (padded), logical H —
        so slicing alone can't extract them."""
        def extract(arr):
            if arr.ndim == 1:
                return np.concatenate(
                    [arr[gb * pH : gb * pH + H] for gb in range(4)]
                ).copy()
            r = arr[:row_l] if row_l else arr
            return np.concatenate(
                [r[:, gb * pH : gb * pH + H] for gb in range(4)], axis=1
            ).copy()

        def insert(view, t):
            view.zero_()
            if view.dim() == 1:
                for gb in range(4):
                    view[gb * pH : gb * pH + H].copy_(
                        t[gb * H : (gb + 1) * H]
                    )
            else:
                rl = row_l if row_l else view.shape[0]
                for gb in range(4):
                    view[:rl, gb * pH : gb * pH + H].copy_(
                        t[:, gb * H : (gb + 1) * H]
                    )

        return extract, insert

    def _declare_params(self):
        spec = self.spec
        lstm_layers = [l for l in spec.layers if l.kind == "lstm"]
        # cell activation each layer runs, beside lstm_meta (a spec
        # saved before the kernels took one runs tanh throughout)
        self.lstm_acts = spec.lstm_activations()
        if self.pad8 and "sigmoid" in self.lstm_acts and any(
            n % 8 for n in [spec.n_features] + [l.units for l in lstm_layers]
        ):
            # sigmoid(0) != 0: pad units would not be inert (see
            # pad_enabled), so this pack keeps its logical dims
            self.pad8 = False
            self._pad = lambda n: int(n)
        p = self._pad
        self.lstm_meta = []          # PHYSICAL (fin, H, return_sequences)
        self.lstm_meta_logical = []  # logical dims for serialization
        fin_l = spec.n_features
        dense_layers = [l for l in spec.layers if l.kind == "dense"]
        assert len(dense_layers) == 1, "LSTM spec needs exactly one output dense layer"
        self._logical_in = fin_l
        for i, layer in enumerate(lstm_layers):
            H_l = layer.units
            fin, H = p(fin_l), p(H_l)
            # each regularizer covers all four gates of its tensor
            regs = layer.weight_regs()
            self.store.declare(f"Wx{i}", (self.G, fin, 4 * H),
                               logical=(self.G, fin_l, 4 * H_l),
                               reg=regs["kernel"])
            self.store.declare(f"Wh{i}", (self.G, H, 4 * H),
                               logical=(self.G, H_l, 4 * H_l),
                               reg=regs["recurrent"])
            self.store.declare(f"bl{i}", (self.G, 4 * H),
                               logical=(self.G, 4 * H_l), reg=regs["bias"])
            if H != H_l or fin != fin_l:
                self._extractors[f"Wx{i}"] = self._gate_converters(
                    H_l, H, fin_l
                )
                self._extractors[f"Wh{i}"] = self._gate_converters(
                    H_l, H, H_l
                )
                self._extractors[f"bl{i}"] = self._gate_converters(
                    H_l, H, None
                )
            self.lstm_meta.append((fin, H, layer.return_sequences))
            self.lstm_meta_logical.append((fin_l, H_l, layer.return_sequences))
            fin_l = H_l
        out_layer = dense_layers[0]
        self._logical_out = out_layer.units
        self.dense_meta = (p(fin_l), p(out_layer.units), out_layer.activation)
        self.dense_meta_logical = (fin_l, out_layer.units, out_layer.activation)
        out_regs = out_layer.weight_regs()
        self.store.declare("Wd", (self.G, p(fin_l), p(out_layer.units)),
                           logical=(self.G, fin_l, out_layer.units),
                           reg=out_regs["kernel"])
        self.store.declare("bd", (self.G, p(out_layer.units)),
                           logical=(self.G, out_layer.units),
                           reg=out_regs["bias"])

    def _init_weights(self):
        # draw the LOGICAL matrices in the same RNG order as the
        # unpadded CPU pack (seed determinism across devices), then
        # scatter into the padded gate blocks
        for g in range(self.G):
            gen = torch.Generator().manual_seed(int(self.seeds[g]) & 0x7FFFFFFF)
            for i, (fin_l, H_l, _rs) in enumerate(self.lstm_meta_logical):
                _pfin, pH, _ = self.lstm_meta[i]
                wx = _glorot_uniform((fin_l, 4 * H_l), gen)
                wh = torch.cat(
                    [_orthogonal((H_l, H_l), gen) for _ in range(4)], dim=1
                )
                b = torch.zeros(4 * H_l)
                b[H_l : 2 * H_l] = 1.0  # unit forget-gate bias (Keras)
                self._insert_logical(
                    f"Wx{i}", self.store.views[f"Wx{i}"][g], wx.numpy()
                )
                self._insert_logical(
                    f"Wh{i}", self.store.views[f"Wh{i}"][g], wh.numpy()
                )
                self._insert_logical(
                    f"bl{i}", self.store.views[f"bl{i}"][g], b.numpy()
                )
            fin_l, fout_l, _act = self.dense_meta_logical
            wd = _glorot_uniform((fin_l, fout_l), gen)
            self.store.views["Wd"][g][:fin_l, :fout_l].copy_(wd)

    # ---- sequence forward/backward ------------------------------------
    def _scan_modes(self, B: Optional[int] = None) -> List[str]:
        """How each layer runs, as the scan planner answers
        (``ops.lstm_layer_mode``): "fused" (one scan launch per layer
        and direction, the x-side GEMM inside it), "two_step" (x-GEMM,
        then one scan launch) or "per_step" (per-timestep kernels). A
        stack runs the scans only when every layer has one — and, for
        big-H stacks, the scan grid fills the chip: the round-2 GPU A/B
        at dims 256/128/64 measured fused 14% SLOWER at G=16 (128
        workgroups on 256 CUs) and 7% faster at G=64 (512 WGs) — so one
        per_step layer sends the whole stack per timestep."""
        n = len(self.lstm_meta)
        if self.device.type != "cuda":
            return ["per_step"] * n
        rows = B if B is not None else 256
        modes = [
            ops.lstm_layer_mode(self.G, rows, H, fin, act)
            for (fin, H, _rs), act in zip(self.lstm_meta, self.lstm_acts)
        ]
        return ["per_step"] * n if "per_step" in modes else modes

    def _use_fused(self, B: Optional[int] = None) -> bool:
        return "per_step" not in self._scan_modes(B)

    def _layer_fwd_steps(self, li, seq, keep):
        """One layer per timestep: x-GEMM, then T x (h@Wh, gate math)."""
        G, B, T, fin = seq.shape
        H = self.lstm_meta[li][1]
        Wx = self.store.cviews[f"Wx{li}"]
        Wh = self.store.cviews[f"Wh{li}"]
        b = self.store.views[f"bl{li}"]
        gates_all = ops.grouped_linear_fwd(
            seq.reshape(G, B * T, fin), Wx, b, "linear"
        ).view(G, B, T, 4 * H)
        lp = dict(dtype=self.compute_dtype, device=self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        h = torch.zeros(G, B, H, **lp)
        c = torch.zeros(G, B, H, **f32)
        hs = torch.empty(G, B, T, H, **lp)
        cs = torch.empty(G, B, T, H, **f32) if keep else None
        gacts = torch.empty(G, B, T, 4 * H, **lp) if keep else None
        for t in range(T):
            gates = gates_all[:, :, t].contiguous()
            ops.grouped_gemm_acc(h, Wh, gates)
            h, c, gact = ops.lstm_pointwise_fwd(gates, c, self.lstm_acts[li])
            hs[:, :, t] = h
            if keep:
                cs[:, :, t] = c
                gacts[:, :, t] = gact
        return hs, cs, gacts

    def _layer_fwd_scan(self, li, mode, seq, keep):
        """One layer in one scan launch. "fused" computes the x-side
        gate GEMM INSIDE the scan (no xW HBM round trip — the fleet's
        scans are bandwidth-bound) and skips the cs/gacts stores on
        inference passes; "two_step" runs the x-GEMM, then the scan."""
        G, B, T, fin = seq.shape
        H = self.lstm_meta[li][1]
        Wx = self.store.cviews[f"Wx{li}"]
        Wh = self.store.cviews[f"Wh{li}"]
        b = self.store.views[f"bl{li}"]
        if mode == "fused":
            out = ops.lstm_seq_fwd_fused(seq, Wx, Wh, b, store_aux=keep,
                                         act=self.lstm_acts[li])
            return (out[0], out[1], out[2]) if keep else (out[0], None, None)
        xW = ops.grouped_linear_fwd(
            seq.reshape(G, B * T, fin), Wx, b, "linear"
        ).view(G, B, T, 4 * H)
        hs, cs, gacts = ops.lstm_seq_fwd(xW, Wh)
        return (hs, cs, gacts) if keep else (hs, None, None)

    def _forward_seq(self, Xw: torch.Tensor, keep: bool, modes=None):
        """Xw: [G, B, T, F]. Returns (y, cache). ``modes``: the answer
        of ``_scan_modes`` where the caller already has it."""
        if modes is None:
            modes = self._scan_modes(Xw.shape[1])
        seq = Xw
        cache = []
        for li, mode in enumerate(modes):
            if mode == "per_step":
                hs, cs, gacts = self._layer_fwd_steps(li, seq, keep)
            else:
                hs, cs, gacts = self._layer_fwd_scan(li, mode, seq, keep)
            cache.append(
                dict(seq_in=seq if keep else None, hs=hs, cs=cs, gacts=gacts)
            )
            seq = hs
        h_last = seq[:, :, -1].contiguous()
        fin, fout, act = self.dense_meta
        y = ops.grouped_linear_fwd(
            h_last, self.store.cviews["Wd"], self.store.views["bd"], act
        )
        if keep:
            cache.append(dict(h_last=h_last, y=y))
        return y, cache

    def predict_windows(self, Xw: torch.Tensor) -> torch.Tensor:
        Xc = self._to_compute(Xw)
        if self.pad8 and Xc.shape[-1] == self._logical_in:
            Xc = self._pad_features(Xc, self._logical_in)
        y, _ = self._forward_seq(Xc, keep=False)
        return y[..., : self._logical_out]

    def eval_batch_stats(self, Xw, Tb):
        Xw, Tb = self._pad_io(Xw, Tb)
        y, _ = self._forward_seq(self._to_compute(Xw), keep=False)
        loss, _, correct = self._loss_bwd(y, Tb, want_grad=False)
        return loss, correct

    def _head_bwd(self, head, dY):
        """Output dense layer backward: stores dWd / dbd, returns the
        gradient on the last hidden state."""
        fin, fout, act = self.dense_meta
        dZ = ops.act_l1_bwd(dY, head["y"], act, 0.0)
        dWd, dbd = ops.grouped_linear_wgrad(head["h_last"], dZ)
        self.store.gviews["Wd"].copy_(dWd)
        self.store.gviews["bd"].copy_(dbd)
        return ops.grouped_linear_bwd_data(dZ, self.store.cviews["Wd"])

    def _layer_bwd_steps(self, li, lc, d_in, last_only):
        """BPTT through one layer per timestep: returns dG [G,B,T,4H]."""
        cs, gacts = lc["cs"], lc["gacts"]
        G, B, T, H = cs.shape
        Wh = self.store.cviews[f"Wh{li}"]
        lp = dict(dtype=self.compute_dtype, device=self.device)
        dG = torch.empty(G, B, T, 4 * H, **lp)
        dh_carry = torch.zeros(G, B, H, **lp)
        dc_carry = torch.zeros(G, B, H, dtype=torch.float32, device=self.device)
        for t in range(T - 1, -1, -1):
            dh_t = dh_carry
            if not last_only:
                dh_t = dh_t + d_in[:, :, t]
            elif t == T - 1:
                dh_t = dh_t + d_in
            c_prev = cs[:, :, t - 1] if t > 0 else torch.zeros_like(dc_carry)
            dgates, dc_carry = ops.lstm_pointwise_bwd(
                dh_t, dc_carry, gacts[:, :, t], cs[:, :, t], c_prev,
                self.lstm_acts[li],
            )
            dG[:, :, t] = dgates
            dh_carry = ops.grouped_linear_bwd_data(dgates, Wh)
        return dG

    def _store_layer_grads(self, li, lc, dG_flat, T):
        """Batched weight grads over all (B, T) rows, in one combined
        pass: dZ (dG) staged once for both weight grads; dWh reads
        h_{t-1} via in-kernel shifted addressing."""
        G, BT, _ = dG_flat.shape
        dWx, dWh, dbl = ops.grouped_wgrad_xh(
            lc["seq_in"].reshape(G, BT, -1), lc["hs"], dG_flat, T
        )
        self.store.gviews[f"Wx{li}"].copy_(dWx)
        self.store.gviews[f"Wh{li}"].copy_(dWh)
        self.store.gviews[f"bl{li}"].copy_(dbl)

    def train_batch(self, Xw, Tb) -> torch.Tensor:
        Xw, Tb = self._pad_io(Xw, Tb)
        G, B, T, _ = Xw.shape
        modes = self._scan_modes(B)
        y, cache = self._forward_seq(Xw, keep=True, modes=modes)
        loss, dY, self.last_correct = self._loss_bwd(y, Tb)
        dh_last = self._head_bwd(cache[-1], dY)

        # BPTT through the LSTM stack
        dSeq: Optional[torch.Tensor] = None  # grad on layer output sequence
        for li in range(len(self.lstm_meta) - 1, -1, -1):
            fin, H, rs = self.lstm_meta[li]
            lc = cache[li]
            Wh = self.store.cviews[f"Wh{li}"]
            Wx = self.store.cviews[f"Wx{li}"]
            last_only = dSeq is None
            d_in = dh_last if last_only else dSeq
            next_dSeq = None
            if modes[li] == "per_step":
                dG = self._layer_bwd_steps(li, lc, d_in, last_only)
            elif li > 0 and modes[li] == "fused":
                # the dSeq GEMM rides inside the reverse scan
                dG, next_dSeq = ops.lstm_seq_bwd_fused(
                    d_in, lc["gacts"], lc["cs"], Wh, Wx, last_only,
                    act=self.lstm_acts[li],
                )
            else:
                dG = ops.lstm_seq_bwd(
                    d_in, lc["gacts"], lc["cs"], Wh, last_only,
                    act=self.lstm_acts[li],
                )
            dG_flat = dG.view(G, B * T, 4 * H)
            self._store_layer_grads(li, lc, dG_flat, T)
            # free this layer's BPTT cache before descending: the
            # allocator reuses it for the next layer's dSeq/transients
            # (whole-batch caches are the memory ceiling at G~100+).
            cache[li] = None
            del lc, dG, d_in
            if li > 0:
                dSeq = (
                    next_dSeq
                    if next_dSeq is not None
                    else ops.grouped_linear_bwd_data(dG_flat, Wx).view(
                        G, B, T, fin
                    )
                )
            del dG_flat

        self.store.optimizer_step()
        return loss

    # ---- windowed fit/predict over a series ---------------------------
    @property
    def lookback(self) -> int:
        return self.spec.lookback_window

    @property
    def lookahead(self) -> int:
        return self.spec.lookahead

    def n_windows(self, N: int) -> int:
        return N - self.lookback + 1 - self.lookahead

    _n_samples = n_windows

    def _gather_batch(self, X, Y, idx):
        """idx: [G, B] window start indices. Builds [G,B,T,F] window
        tensors (K7 HIP gather kernel on GPU) and [G,B,Fo] targets
        straight from the series."""
        G, N, F = X.shape
        Fo = Y.shape[2]
        B = idx.shape[1]
        T = self.lookback
        Xw = ops.window_gather(X, idx, T)
        trow = idx + (T - 1 + self.lookahead)
        Tb = Y.gather(1, trow.unsqueeze(-1).expand(G, B, Fo))
        return Xw, Tb

    def predict(self, X: torch.Tensor, batch_size: int = 4096) -> torch.Tensor:
        """X: [G, N, F] series → [G, n_windows, Fo] predictions
        (offset-aligned like the reference: output starts at row
        lookback-1+lookahead)."""
        X = self._to_compute(X)
        if self.pad8:
            X = self._pad_features(X, self._logical_in)
        G, N, F = X.shape
        nw = self.n_windows(N)
        outs = []
        dummyY = X.new_zeros(G, N, self.dense_meta[1])
        for s in range(0, nw, batch_size):
            idx = (
                torch.arange(s, min(s + batch_size, nw), device=self.device)
                .unsqueeze(0)
                .expand(G, -1)
            )
            Xw, _ = self._gather_batch(X, dummyY, idx)
            outs.append(self.predict_windows(Xw))
        return torch.cat(outs, dim=1)
