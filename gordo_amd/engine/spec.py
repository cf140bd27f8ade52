"""
ModelSpec — the device-engine model description.

The factory functions in ``machine/model/factories`` (the analog of the
reference's Keras model builders, feedforward_autoencoder.py /
lstm_autoencoder.py) produce these specs; the packed engine
(``engine/pack.py``) materializes G of them at a time on one GPU.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field, asdict
from typing import Any, Dict, List, Optional, Tuple

logger = logging.getLogger(__name__)


# ---- compile settings -------------------------------------------------
# Keras names and aliases (case-insensitive) -> the engine's canonical
# loss / optimizer names. Anything else raises: a silent fallback to
# Adam/MSE would train a different model than the one configured.
_LOSS_ALIASES = {
    "mse": "mse",
    "mean_squared_error": "mse",
    "meansquarederror": "mse",
    "mae": "mae",
    "mean_absolute_error": "mae",
    "meanabsoluteerror": "mae",
    "huber": "huber",
    "huber_loss": "huber",
    "logcosh": "logcosh",
    "log_cosh": "logcosh",
}
_LOSS_KWARGS = {"huber": {"delta": 1.0}}

# per-optimizer hyperparameters and their Keras 3 defaults
_OPTIMIZER_DEFAULTS: Dict[str, Dict[str, Any]] = {
    "adam": dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999,
                 epsilon=1e-7, amsgrad=False),
    "sgd": dict(learning_rate=0.01, momentum=0.0, nesterov=False),
    "rmsprop": dict(learning_rate=0.001, rho=0.9, momentum=0.0,
                    epsilon=1e-7),
    "adagrad": dict(learning_rate=0.001, initial_accumulator_value=0.1,
                    epsilon=1e-7),
    "adamax": dict(learning_rate=0.001, beta_1=0.9, beta_2=0.999,
                   epsilon=1e-7),
}


# cell activations the LSTM kernels implement (the candidate gate and
# φ(c); the i/f/o gates are always sigmoid). Same rule as above: any
# other name raises instead of silently training tanh.
LSTM_ACTIVATIONS = ("linear", "relu", "sigmoid", "tanh")


def normalize_lstm_activation(name: Any) -> str:
    """Canonical LSTM cell activation; ``None`` is linear, as for Dense.

    >>> normalize_lstm_activation("ReLU"), normalize_lstm_activation(None)
    ('relu', 'linear')
    """
    key = "linear" if name is None else (
        name.lower() if isinstance(name, str) else None
    )
    if key not in LSTM_ACTIVATIONS:
        raise ValueError(
            f"Unsupported LSTM activation {name!r}; supported: "
            f"{sorted(LSTM_ACTIVATIONS)}"
        )
    return key


def _is_off(v: Any) -> bool:
    """Keras optimizer kwargs the engine has no analog for are accepted
    only at their "off" value: None or False themselves (identity — 0
    and 0.0 compare equal to False but are settings, so they raise)."""
    return v is None or v is False


def normalize_loss(name: Any) -> str:
    """Canonical loss name (``mse``/``mae``/``huber``/``logcosh``).

    >>> normalize_loss("mean_squared_error"), normalize_loss("Huber")
    ('mse', 'huber')
    """
    key = str(name).rsplit(".", 1)[-1].lower() if isinstance(name, str) else None
    if key not in _LOSS_ALIASES:
        raise ValueError(
            f"Unsupported loss {name!r}; supported: "
            f"{sorted(set(_LOSS_ALIASES.values()))}"
        )
    return _LOSS_ALIASES[key]


def normalize_optimizer(name: Any) -> str:
    """Canonical optimizer name.

    >>> normalize_optimizer("Adam"), normalize_optimizer("RMSprop")
    ('adam', 'rmsprop')
    """
    key = str(name).rsplit(".", 1)[-1].lower() if isinstance(name, str) else None
    if key not in _OPTIMIZER_DEFAULTS:
        raise ValueError(
            f"Unsupported optimizer {name!r}; supported: "
            f"{sorted(_OPTIMIZER_DEFAULTS)}"
        )
    return key


def resolve_loss(loss: Any, loss_kwargs: Optional[Dict[str, Any]] = None
                 ) -> Tuple[str, Dict[str, float]]:
    """(canonical loss, complete kwargs) — raises ValueError on an
    unknown loss or an unknown loss kwarg."""
    kind = normalize_loss(loss)
    params = dict(_LOSS_KWARGS.get(kind, {}))
    for k, v in (loss_kwargs or {}).items():
        if k in ("name", "reduction"):
            if k == "reduction" and v not in (None, "sum_over_batch_size",
                                              "auto"):
                raise ValueError(f"Unsupported loss kwarg reduction={v!r}")
            continue
        if k not in params:
            raise ValueError(f"Unsupported kwarg {k!r} for loss {loss!r}")
        params[k] = float(v)
    if kind == "huber" and not params["delta"] > 0.0:
        raise ValueError(f"huber delta must be > 0, got {params['delta']!r}")
    return kind, params


def resolve_optimizer(optimizer: Any,
                      optimizer_kwargs: Optional[Dict[str, Any]] = None
                      ) -> Tuple[str, Dict[str, Any]]:
    """(canonical optimizer, complete hyperparameters) with Keras 3
    defaults filled in — raises ValueError naming the first kwarg the
    engine cannot honour (clipnorm, weight_decay, centered=True, ...)."""
    kind = normalize_optimizer(optimizer)
    params = dict(_OPTIMIZER_DEFAULTS[kind])
    for k, v in (optimizer_kwargs or {}).items():
        if k == "name":
            continue
        if k == "lr":
            k = "learning_rate"
        if k not in params:
            if _is_off(v):
                continue  # e.g. centered=False, clipnorm=None
            raise ValueError(
                f"Unsupported optimizer kwarg {k!r} for {optimizer!r}"
            )
        if isinstance(params[k], bool):
            if not isinstance(v, (bool, int)) or v not in (0, 1):
                raise ValueError(
                    f"Unsupported value for optimizer flag {k!r}: {v!r}"
                )
            params[k] = bool(v)
        else:
            if isinstance(v, (dict, list, tuple, str)) or v is None:
                raise ValueError(
                    f"Unsupported value for optimizer kwarg {k!r}: {v!r}"
                )
            params[k] = float(v)
    return kind, params


def parse_compile_kwargs(compile_kwargs: Optional[Dict[str, Any]]
                         ) -> Tuple[str, Dict[str, Any]]:
    """The factories' ``compile_kwargs``: returns (loss, loss_kwargs),
    the loss name as the user wrote it. ``loss`` is a string or a
    single-key dict with kwargs; ``metrics`` may only ask for accuracy
    (history always carries it)."""
    ck = dict(compile_kwargs or {})
    loss = ck.pop("loss", None)
    loss_kwargs: Dict[str, Any] = {}
    if loss is None:
        loss = "mse"
    elif isinstance(loss, dict) and len(loss) == 1:
        key = next(iter(loss))
        loss_kwargs = dict(loss[key] or {})
        loss = str(key).rsplit(".", 1)[-1]
    elif not isinstance(loss, str):
        raise ValueError(f"Unparsable compile entry loss={loss!r}")
    metrics = ck.pop("metrics", None)
    if isinstance(metrics, str):
        metrics = [metrics]
    for m in metrics or []:
        if not (isinstance(m, str) and m.lower() in ("accuracy", "acc")):
            raise ValueError(
                f"Unsupported metrics entry {m!r}; only 'accuracy' is "
                "computed by the engine"
            )
    for k, v in ck.items():
        # settings that do not change the trained model pass through
        if k in ("run_eagerly", "steps_per_execution", "jit_compile",
                 "auto_scale_loss"):
            continue
        if v is None:
            continue
        raise ValueError(f"Unsupported compile kwarg {k!r}")
    resolve_loss(loss, loss_kwargs)
    return loss, loss_kwargs


def _freeze(v: Any) -> Any:
    if isinstance(v, dict):
        return tuple(sorted((k, _freeze(x)) for k, x in v.items()))
    if isinstance(v, (list, tuple)):
        return tuple(_freeze(x) for x in v)
    return v


# ---- weight regularizers ----------------------------------------------
# LayerSpec field pairs, in the order arch_key and to_dict list them
_REG_FIELDS = ("kernel_l1", "kernel_l2", "bias_l1", "bias_l2",
               "recurrent_l1", "recurrent_l2")
# Keras regularizer names (last path component, lower-cased) -> the
# (l1, l2) defaults of that class; None: the class has no such term
_REGULARIZER_DEFAULTS = {
    "l1l2": (0.0, 0.0),
    "l1": (0.01, None),
    "l2": (None, 0.01),
    "l1_l2": (0.01, 0.01),
}


def _reg_coefficient(owner: str, key: str, v: Any) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(
            f"Unsupported {owner} coefficient {key}={v!r}: not a number"
        )
    v = float(v)
    if not (v >= 0.0 and v != float("inf")):
        raise ValueError(
            f"Unsupported {owner} coefficient {key}={v!r}: must be a "
            "finite number >= 0"
        )
    return v


def parse_weight_regularizer(reg_def: Any, owner: str = "regularizer"
                             ) -> Tuple[float, float]:
    """(l1, l2) of a Keras weight regularizer definition: ``None``; one
    of the strings ``"l1"``, ``"l2"``, ``"l1_l2"`` (0.01 each); a
    single-key dict ``{"...L1L2": {"l1": a, "l2": b}}`` (defaults 0, 0),
    ``{"...L1": {"l1": a}}``, ``{"...L2": {"l2": b}}`` (default 0.01) or
    ``{"...l1_l2": {...}}`` (defaults 0.01, 0.01), the class name
    case-insensitive; or a plain ``{"l1": a, "l2": b}``. Anything else
    raises ValueError naming the offender (``owner`` says which
    setting it came from).

    >>> parse_weight_regularizer({"keras.regularizers.L1L2": {"l1": 0.2}})
    (0.2, 0.0)
    >>> parse_weight_regularizer("l2")
    (0.0, 0.01)
    """
    if reg_def is None:
        return 0.0, 0.0
    if isinstance(reg_def, str):
        name = reg_def.rsplit(".", 1)[-1].lower()
        if name not in ("l1", "l2", "l1_l2"):
            raise ValueError(f"Unsupported {owner} {reg_def!r}")
        l1, l2 = _REGULARIZER_DEFAULTS[name]
        return l1 or 0.0, l2 or 0.0
    if not isinstance(reg_def, dict) or not reg_def:
        raise ValueError(f"Unsupported {owner} {reg_def!r}")
    if all(k in ("l1", "l2") for k in reg_def):
        # the plain form; a lone key whose value is a dict is the
        # class form with a lower-case name: {"l1": {"l1": a}}
        lone = next(iter(reg_def.values())) if len(reg_def) == 1 else 0
        if not isinstance(lone, dict):
            return (
                _reg_coefficient(owner, "l1", reg_def.get("l1", 0.0)),
                _reg_coefficient(owner, "l2", reg_def.get("l2", 0.0)),
            )
    if len(reg_def) != 1:
        bad = sorted(str(k) for k in reg_def if k not in ("l1", "l2"))
        raise ValueError(
            f"Unsupported {owner} {reg_def!r}: unknown key {bad[0]!r}"
        )
    cls_name, kwargs = next(iter(reg_def.items()))
    name = str(cls_name).rsplit(".", 1)[-1].lower()
    if name not in _REGULARIZER_DEFAULTS:
        raise ValueError(
            f"Unsupported {owner} class {cls_name!r}; supported: L1, L2, "
            "L1L2, l1_l2"
        )
    if kwargs is not None and not isinstance(kwargs, dict):
        raise ValueError(
            f"Unsupported {owner} arguments {kwargs!r} for {cls_name!r}"
        )
    out = dict(zip(("l1", "l2"), _REGULARIZER_DEFAULTS[name]))
    for k, v in (kwargs or {}).items():
        if k not in out or out[k] is None:
            raise ValueError(
                f"Unsupported {owner} key {k!r} for {cls_name!r}"
            )
        out[k] = _reg_coefficient(owner, k, v)
    return out["l1"] or 0.0, out["l2"] or 0.0


@dataclass
class LayerSpec:
    kind: str  # "dense" | "lstm"
    units: int
    activation: str = "tanh"
    l1_activity: float = 0.0  # L1 activity regularizer weight (dense)
    return_sequences: bool = True  # lstm only
    # weight regularizers (Keras kernel_ / bias_ / recurrent_regularizer):
    # each adds l1 sum|w| + l2 sum w^2 over its tensor to the model's
    # loss. The recurrent pair is legal only on lstm.
    kernel_l1: float = 0.0
    kernel_l2: float = 0.0
    bias_l1: float = 0.0
    bias_l2: float = 0.0
    recurrent_l1: float = 0.0
    recurrent_l2: float = 0.0

    def __post_init__(self):
        for name in _REG_FIELDS:
            setattr(self, name, _reg_coefficient(
                f"{self.kind} layer", name, getattr(self, name)
            ))
        if self.kind != "lstm" and (self.recurrent_l1 or self.recurrent_l2):
            raise ValueError(
                f"recurrent_regularizer on a {self.kind} layer: only LSTM "
                "layers have a recurrent kernel"
            )

    def __setstate__(self, state):
        # a layer pickled before the weight regularizers existed
        self.__dict__.update(state)
        for name in _REG_FIELDS:
            self.__dict__.setdefault(name, 0.0)

    def weight_regs(self) -> Dict[str, Tuple[float, float]]:
        """(l1, l2) per tensor role: kernel, recurrent, bias."""
        return {
            "kernel": (self.kernel_l1, self.kernel_l2),
            "recurrent": (self.recurrent_l1, self.recurrent_l2),
            "bias": (self.bias_l1, self.bias_l2),
        }

    def to_dict(self) -> Dict[str, Any]:
        return _layer_dict(asdict(self))

    @classmethod
    def from_dict(cls, d) -> "LayerSpec":
        return cls(**d)


def _layer_dict(d: Dict[str, Any]) -> Dict[str, Any]:
    """A layer's dict without the regularizer fields when all are zero:
    an unregularized layer's dict is what it was before they existed."""
    if not any(d[name] for name in _REG_FIELDS):
        for name in _REG_FIELDS:
            del d[name]
    return d


@dataclass
class ModelSpec:
    model_type: str  # "feedforward" | "lstm"
    n_features: int
    n_features_out: int
    layers: List[LayerSpec] = field(default_factory=list)
    lookback_window: int = 1  # lstm path
    lookahead: int = 0  # 0 = autoencoder, 1 = one-step forecast
    loss: str = "mse"
    optimizer: str = "Adam"
    optimizer_kwargs: Dict[str, Any] = field(default_factory=dict)
    loss_kwargs: Dict[str, Any] = field(default_factory=dict)
    # 1: LSTM layers run their configured activation. 0 (specs saved
    # before the kernels took one): every LSTM layer was trained as
    # tanh whatever its stored name says, and keeps running tanh.
    lstm_act_version: int = 1

    def __post_init__(self):
        # unsupported compile settings fail HERE, when the spec is
        # built, before any device work. The stored loss/optimizer
        # strings stay exactly as the user wrote them.
        self.optimizer_kwargs = dict(self.optimizer_kwargs or {})
        self.loss_kwargs = dict(self.loss_kwargs or {})
        resolve_loss(self.loss, self.loss_kwargs)
        resolve_optimizer(self.optimizer, self.optimizer_kwargs)
        for layer in self.layers:
            if layer.kind == "lstm":
                normalize_lstm_activation(layer.activation)

    def __setstate__(self, state):
        # specs pickled inside estimators saved before ``loss_kwargs``
        # / ``lstm_act_version`` existed restore without them
        # (unpickling bypasses __init__)
        self.__dict__.update(state)
        self.__dict__.setdefault("loss_kwargs", {})
        self.__dict__.setdefault("lstm_act_version", 0)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_lstm_act_warned", None)
        return state

    def to_dict(self) -> Dict[str, Any]:
        d = asdict(self)
        d["layers"] = [_layer_dict(x) for x in d["layers"]]
        if not d["loss_kwargs"]:
            del d["loss_kwargs"]
        if d["lstm_act_version"] == 1:
            del d["lstm_act_version"]
        return d

    @classmethod
    def from_dict(cls, d) -> "ModelSpec":
        d = dict(d)
        d["layers"] = [LayerSpec.from_dict(x) for x in d.get("layers", [])]
        return cls(**d)

    # ---- shape helpers -------------------------------------------------
    def dense_dims(self) -> List[tuple]:
        """[(in, out, act, l1), ...] for a pure-dense spec."""
        assert self.model_type == "feedforward"
        dims = []
        prev = self.n_features
        for layer in self.layers:
            dims.append((prev, layer.units, layer.activation, layer.l1_activity))
            prev = layer.units
        return dims

    def has_weight_regularizers(self) -> bool:
        return any(
            getattr(l, name) for l in self.layers for name in _REG_FIELDS
        )

    def lstm_activations(self) -> List[str]:
        """Canonical cell activation each LSTM layer RUNS, in layer
        order. A version-0 spec runs tanh throughout; the first call
        logs one warning if a stored name says otherwise."""
        names = [
            normalize_lstm_activation(l.activation)
            for l in self.layers if l.kind == "lstm"
        ]
        if self.lstm_act_version >= 1:
            return names
        stale = sorted({n for n in names if n != "tanh"})
        if stale and not self.__dict__.get("_lstm_act_warned"):
            self.__dict__["_lstm_act_warned"] = True
            logger.warning(
                "This model was saved when LSTM layers ignored their "
                "configured activation (%s): it was trained as tanh and "
                "keeps running tanh. Rebuild it to train the configured "
                "activation.", ", ".join(stale),
            )
        return ["tanh"] * len(names)

    def arch_key(self) -> tuple:
        """Hashable architecture key — models with equal keys can share
        one pack (grouped-GEMM batch)."""
        return (
            self.model_type,
            self.n_features,
            self.n_features_out,
            tuple(
                (l.kind, l.units, l.activation, l.l1_activity,
                 l.return_sequences)
                # per tensor, not per model: differently regularized
                # models do not share a pack
                + tuple(getattr(l, name) for name in _REG_FIELDS)
                for l in self.layers
            ),
            self.lookback_window,
            self.lookahead,
            self.lstm_act_version,
            # normalised, defaults filled in: "adam"/"Adam" and
            # "mse"/"mean_squared_error" share a pack
            self.loss_kind,
            _freeze(self.loss_params),
            self.optimizer_kind,
            _freeze(self.optimizer_params),
        )

    # ---- compile settings (normalised) ---------------------------------
    @property
    def loss_kind(self) -> str:
        return normalize_loss(self.loss)

    @property
    def loss_params(self) -> Dict[str, float]:
        return resolve_loss(self.loss, self.loss_kwargs)[1]

    @property
    def optimizer_kind(self) -> str:
        return normalize_optimizer(self.optimizer)

    @property
    def optimizer_params(self) -> Dict[str, Any]:
        """Complete hyperparameters of the configured optimizer (Keras
        3 defaults filled in, ``lr`` folded into ``learning_rate``)."""
        return resolve_optimizer(self.optimizer, self.optimizer_kwargs)[1]

    @property
    def adam_params(self):
        kw = self.optimizer_kwargs or {}
        return dict(
            lr=float(kw.get("lr", kw.get("learning_rate", 0.001))),
            beta1=float(kw.get("beta_1", 0.9)),
            beta2=float(kw.get("beta_2", 0.999)),
            eps=float(kw.get("epsilon", 1e-7)),  # keras default epsilon
        )
